"""The shifted warm start (rn_shift_warm_start, rn_set_shift_map, rn_get_shift_map) through the layers that need no GPU: the entry points in
the header, in the library's exports and in the Python binding; null contexts refused at the boundary; the optional "warmStart" key of the
controller configuration; the host classes' members.  On a GPU the program tests/cpp/test_shift_warm_start.cpp runs a closed loop of three
control steps through SmpcController: the key against the calls by hand, "keep" against the identity as a caller's map."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rapidnet_amd import build, capi, synth

NEW = ("rn_shift_warm_start", "rn_set_shift_map", "rn_get_shift_map")
RN_E_ARG = -1


def _files(tmp_path, keep="keep", shift="shift"):
    plain = synth.write_problem(synth.make_problem("small", max_iterations=60), str(tmp_path))
    for fname, value in (("controllerKeepConfig.json", keep), ("controllerShiftConfig.json", shift)):
        cfg = json.load(open(plain))
        cfg["warmStart"] = value
        json.dump(cfg, open(os.path.join(str(tmp_path), fname), "w"))


def test_program_is_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_SHIFT_WARM_START)


def test_new_symbols_are_declared_exported_bound_and_described():
    hdr = open(os.path.join(ROOT, "include", "rapidnet.h")).read()
    declared = set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.load()
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    comment = hdr[: hdr.index("int rn_shift_warm_start(")].rsplit("/* Extension", 1)[1]
    for words in ("SmpcController.cu:1509", "min(r, nc - 1)", "sqrt(p_i / p_m)", "d[stage(m)][c] / d[stage(i)][c]", "RN_E_STATE", "RN_E_ARG", "L-BFGS", "BOTH"):
        assert words in comment, words
    for method in ("shiftWarmStart", "setShiftMap", "getShiftMap"):
        assert hasattr(capi.Solver, method), method
    import inspect

    assert inspect.signature(capi.Solver.shiftWarmStart).parameters["root_child"].default == -1
    for cls, member in (("Engine.hpp", "shiftWarmStart"), ("Engine.hpp", "setShiftMap"), ("Engine.hpp", "getShiftMap"), ("SmpcController.hpp", "shiftWarmStart"),
                        ("DataModel.hpp", "getWarmStart")):
        assert member in open(os.path.join(ROOT, "rapidnet_amd", "csrc", "host", cls)).read(), (cls, member)
    assert "k_shift_duals<0>" in open(os.path.join(ROOT, "rapidnet_amd", "csrc", "instantiations", "dual.inc")).read()


def test_null_contexts_are_refused_without_a_gpu():
    """(ranges, sizes and the state rules need a live context, hence a device: tests/test_gpu_shift_warm_start.py)"""
    lib = capi.load()
    m = np.full(4, 7, np.int32)
    assert lib.rn_shift_warm_start(None, 0) == RN_E_ARG and lib.rn_shift_warm_start(None, -1) == RN_E_ARG
    assert lib.rn_set_shift_map(None, 4, m.ctypes.data) == RN_E_ARG and lib.rn_set_shift_map(None, 0, None) == RN_E_ARG
    assert lib.rn_get_shift_map(None, 0, 4, m.ctypes.data) == RN_E_ARG and (m == 7).all()


def test_key_is_parsed_and_an_absent_key_means_off(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = subprocess.run([build.TEST_SHIFT_WARM_START, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "plain: warmStart off" in r.stdout and "keep: warmStart keep" in r.stdout and "shift: warmStart shift" in r.stdout, r.stdout
    _files(tmp_path, keep="off")
    r = subprocess.run([build.TEST_SHIFT_WARM_START, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "keep: warmStart off" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("value", ["shifted", "on", ""])
def test_an_unknown_value_of_the_key_is_refused(tmp_path, value):
    build.build_host()
    _files(tmp_path, shift=value)
    r = subprocess.run([build.TEST_SHIFT_WARM_START, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "warmStart must be" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.gpu
def test_shift_warm_start_cpp(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = subprocess.run([build.TEST_SHIFT_WARM_START, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_shift_warm_start failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "shift warm start: all checks passed" in r.stdout
    nc, best = (int(v) for v in re.search(r"root children: (\d+), most probable: (\d+)", r.stdout).groups())
    prob = np.asarray(synth.make_problem("small")["tree"]["probNode"], float)
    assert nc == 3 and best == int(np.argmax(prob[1:4]))
