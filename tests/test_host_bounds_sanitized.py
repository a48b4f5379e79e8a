"""The host arithmetic behind rn_set_bounds / rn_get_bounds (rapidnet_amd/csrc/bounds.hpp, plain C++: rows and strides of a granularity, the
validation of the caller's values, the y order of the tables) under AddressSanitizer and UBSan on the CPU, as a stand-alone program
(tests/cpp/bounds_sanitize.cpp): 300 random shapes, the three granularities each."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_bounds_arithmetic_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "bounds_sanitize")
    src = os.path.join(ROOT, "tests", "cpp", "bounds_sanitize.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "bounds runs 900" in out.stdout
