"""The column-mask arithmetic of k_stream_gemv's walk (csrc/stream_bits.hpp, stream_mask_bits: the G or G / 2 bits of a span or half-span out of
sh_nz) against a bit-by-bit loop, in a stand-alone host program (tests/cpp/test_stream_bits.cpp): runs that straddle two words, runs shorter
than a word, the zero pad word.  And the half-span hook and knob through the layers that need no GPU."""
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from rapidnet_amd import build, capi


def test_mask_bits_equal_a_bit_by_bit_loop():
    build.build_host()
    assert os.path.exists(build.TEST_STREAM_BITS)
    r = subprocess.run([build.TEST_STREAM_BITS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "all equal the bit-by-bit loop" in r.stdout, r.stdout


def test_hook_and_knob_are_declared_exported_and_bound():
    dbg = open(os.path.join(ROOT, "include", "rapidnet_debug.h")).read()
    lib = capi.load()
    name = "rn_debug_stream_units"
    assert name in set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", dbg)) and name in capi.SYMBOLS and hasattr(lib, name)
    assert hasattr(capi.Solver, "streamUnits")
    m = re.search(r"RN_KNOB_STREAM_HALF = (\d+)", dbg)
    assert m and capi.KNOBS["stream_half"] == int(m.group(1))
    assert int(re.search(r"RN_KNOB_COUNT = (\d+)", dbg).group(1)) == len(capi.KNOBS)
    out = np.zeros(3, dtype=np.int64)
    assert lib.rn_debug_stream_units(None, out.ctypes.data) == -1      # RN_E_ARG: no context
