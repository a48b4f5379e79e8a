"""The momentum restart (rn_set_restart) through the layers that need no GPU: the entry points in the headers, in the library's exports and in the
Python binding; argument validation at the boundary; the optional "momentumRestart" key of the controller configuration
(tests/cpp/test_restart.cpp); and the numpy restatement of the restart on the CPU oracle (tests/restart_oracle.py) that the GPU tests compare
against, pinned to the figures the feature was proposed with.  On a GPU the program's controllers restart a control step
(SmpcController::getRestartsRun) and agree with the C-ABI route."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import restart_oracle as ro
from conftest import ROOT
from oracle.oracle import Oracle
from rapidnet_amd import build, capi, synth

NEW = ("rn_set_restart", "rn_get_restart", "rn_get_restart_info")
HOOK = "rn_debug_restart_test"


def _files(tmp_path, value="gradient", max_iterations=400):
    plain = synth.write_problem(synth.make_problem("small", max_iterations=max_iterations, feasible=True), str(tmp_path))
    cfg = json.load(open(plain))
    cfg["momentumRestart"] = value
    json.dump(cfg, open(os.path.join(str(tmp_path), "controllerRestartConfig.json"), "w"))


def test_program_is_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_RESTART)


def test_new_symbols_are_declared_exported_bound_and_cited():
    hdr = open(os.path.join(ROOT, "include", "rapidnet.h")).read()
    dbg = open(os.path.join(ROOT, "include", "rapidnet_debug.h")).read()
    declared = set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.load()
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
        comment = hdr[: hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "SmpcController.cu:1500-1525" in comment and ":535-557" in comment, name
    assert "RN_RESTART_OFF = 0" in hdr and "RN_RESTART_GRADIENT = 1" in hdr
    assert HOOK in set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", dbg)) and HOOK not in declared and HOOK in capi.SYMBOLS and hasattr(lib, HOOK)
    for method in ("setRestart", "restart", "last_restarts", "debugRestartTest"):
        assert hasattr(capi.Solver, method), method
    import inspect

    assert inspect.signature(capi.Solver.__init__).parameters["restart"].default == "off"
    for cls, member in (("Engine.hpp", "setRestart"), ("Engine.hpp", "getRestart"), ("SmpcController.hpp", "getRestartsRun"), ("DataModel.hpp", "getMomentumRestart")):
        assert member in open(os.path.join(ROOT, "rapidnet_amd", "csrc", "host", cls)).read(), (cls, member)


def test_null_contexts_are_refused_without_a_gpu():
    """(a bad mode and NULL outputs need a live context, hence a device: tests/test_gpu_restart.py and tests/cpp/test_restart.cpp)"""
    lib = capi.load()
    mode, counts, last = C.c_int(5), np.zeros(4, dtype=np.int64), np.zeros(3)
    RN_E_ARG = -1
    assert lib.rn_set_restart(None, capi.RESTART_GRADIENT) == RN_E_ARG
    assert lib.rn_get_restart(None, C.byref(mode)) == RN_E_ARG and mode.value == 5
    assert lib.rn_get_restart_info(None, counts.ctypes.data, last.ctypes.data) == RN_E_ARG
    assert lib.rn_debug_restart_test(None, last.ctypes.data) == RN_E_ARG


def test_key_is_parsed_and_an_absent_key_means_off(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = subprocess.run([build.TEST_RESTART, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "plain: momentumRestart off" in r.stdout and "key: momentumRestart gradient" in r.stdout, r.stdout
    _files(tmp_path, value="off")
    r = subprocess.run([build.TEST_RESTART, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "key: momentumRestart off" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("value", ["residual", "on", ""])
def test_an_unknown_value_of_the_key_is_refused(tmp_path, value):
    build.build_host()
    _files(tmp_path, value=value)
    r = subprocess.run([build.TEST_RESTART, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "momentumRestart must be" in r.stderr, (r.returncode, r.stderr[-2000:])


def _oracle(name):
    p = synth.make_problem(name, feasible=True)
    dh, ah = synth.forecast_at(p["forecast"], 0)
    o = Oracle(p["network"], p["tree"], p["config"])
    o.initialise(dh, ah)
    return o


def test_restatement_on_small_fires_at_180_and_980_and_reaches_the_levels_sooner():
    """The table the feature was proposed with, row `small`: plain APG reaches 1e-2 of the first batch's residual norm at 420 iterations and not
    1e-3 within 1 200; with the gradient test every 20 iterations the momentum restarts at 180 and 980 and the levels are reached at 300 and
    700.  No boundary of the run is marginal: |cos| >= 3e-2 everywhere."""
    plain = ro.restart_loop(_oracle("small"), 1200, 20, restart=False)
    rest = ro.restart_loop(_oracle("small"), 1200, 20, restart=True)
    assert plain["fires"] == [] and plain["tests"] == []
    assert rest["fires"] == [180, 980]
    assert ro.iterations_to(plain["norms"], 20) == [420, None, None]
    assert ro.iterations_to(rest["norms"], 20)[:2] == [300, 700]
    assert len(rest["tests"]) == 60 and len(rest["hist"]) == 1200
    assert min(abs(ro.cosine(t)) for t in rest["tests"]) >= 3e-2
    # up to the first restart the two runs are the same run
    assert np.array_equal(plain["hist"][:180], rest["hist"][:180]) and not np.array_equal(plain["hist"][180:200], rest["hist"][180:200])


def test_restatement_on_tiny_restarts_four_times_and_ends_100x_lower():
    plain = ro.restart_loop(_oracle("tiny"), 600, 20, restart=False)
    rest = ro.restart_loop(_oracle("tiny"), 600, 20, restart=True)
    assert rest["fires"] == [120, 300, 420, 540]
    assert ro.iterations_to(plain["norms"], 20)[0] == 180 and ro.iterations_to(rest["norms"], 20)[0] == 280
    fp, fr = plain["norms"][-1] / plain["norms"][0], rest["norms"][-1] / rest["norms"][0]
    assert 2e-3 < fp < 3.5e-3 and 2e-5 < fr < 3.5e-5, (fp, fr)


def test_restatement_stops_on_a_tolerance_before_it_restarts():
    """The order at a batch end: a solve that stops does not restart in that batch -- and on `small` the restart saves iterations under a
    tolerance.  The library stops on vecPrimalInfs, the larger of two SIGNED residual entries, which on `small` is exactly 0 over the first
    140 iterations: with batches of 20 every solve stops at 20, restart or not.  Batches of 240 put the first boundary behind that prefix
    (residuals at the boundaries, plain: 0.124, 0.027, 0.0149, 0.0106, 0; with the restart that fires at 480: 0.124, 0.027, 0)."""
    plain = ro.restart_loop(_oracle("small"), 1440, 240, restart=False, tol=1e-3)
    rest = ro.restart_loop(_oracle("small"), 1440, 240, restart=True, tol=1e-3)
    assert plain["iterations"] == 1200 and rest["iterations"] == 720
    assert rest["fires"] == [480] and len(rest["tests"]) == 2            # the boundary that stopped was not tested
    assert min(abs(ro.cosine(t)) for t in rest["tests"]) >= 1e-2


def test_gradient_test_of_known_vectors():
    w, yp, y = np.array([3.0, 0.0, 1.0]), np.array([1.0, 0.0, 2.0]), np.array([0.0, 5.0, 2.5])
    g, na2, nb2, mag = ro.gradient_test(w, yp, y)
    assert (g, na2, nb2, mag) == (2.0 * 1.0 + 0.0 + (-1.0) * (-0.5), 5.0, 1.0 + 25.0 + 0.25, 2.5)


@pytest.mark.gpu
def test_restart_key_cpp(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = subprocess.run([build.TEST_RESTART, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_restart failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "momentum restart: all checks passed" in r.stdout
    # small, feasible, forecast 0, 400 iterations: the oracle restarts once, at 180
    assert "restarts: key 1, plain 0 in 400 of 400 iterations" in r.stdout, r.stdout
