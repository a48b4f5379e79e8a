"""Bounds per stage through the C++ class surface (tests/cpp/test_bounds.cpp): SmpcController::updateBounds between two controlAction calls gives,
bit for bit, the control of a controller that set the same bounds before its first step; Engine::setBoundsDevice round-trips through getBounds;
refused calls change nothing and a factor step returns to the network's vectors."""
import os
import subprocess

import pytest

from rapidnet_amd import build, synth


def test_program_is_built_with_the_host_library():
    """compiles against the host headers and links: the new methods and the four C symbols exist"""
    build.build_host()
    assert os.path.exists(build.TEST_BOUNDS)
    r = subprocess.run([build.TEST_BOUNDS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.gpu
def test_bounds_cpp(tmp_path):
    build.build_host()
    p = synth.make_problem("tiny", max_iterations=40)
    synth.write_problem(p, str(tmp_path))
    r = subprocess.run([build.TEST_BOUNDS, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_bounds failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "bounds: all checks passed" in r.stdout
