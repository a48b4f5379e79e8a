"""The stop tolerance through the layers that need no GPU: the optional "stopTolerance" / "stopCheckEvery" keys of the controller configuration
(tests/cpp/test_stop_tolerance.cpp), the new entry points in the header, in the library's exports and in the Python binding; on a GPU the
program's controllers stop a control step early and report the count (SmpcController::getIterationsRun)."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT
from rapidnet_amd import build, capi, synth

NEW = ("rn_apg_solve", "rn_set_stop_tolerance", "rn_get_stop_tolerance", "rn_get_last_solve")


def _files(tmp_path, tol=1e3, every=10, max_iterations=200):
    plain = synth.write_problem(synth.make_problem("small", max_iterations=max_iterations), str(tmp_path))
    cfg = json.load(open(plain))
    cfg["stopTolerance"] = [tol]              # (the reference's files hold every scalar as a one-element array; a bare number is read too)
    cfg["stopCheckEvery"] = every
    json.dump(cfg, open(os.path.join(str(tmp_path), "controllerTolConfig.json"), "w"))


def test_program_is_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_STOP_TOLERANCE)


def test_keys_are_parsed_and_absent_keys_mean_off(tmp_path):
    build.build_host()
    _files(tmp_path, tol=0.125, every=7)
    r = subprocess.run([build.TEST_STOP_TOLERANCE, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "plain: stopTolerance 0 stopCheckEvery 0" in r.stdout and "keys: stopTolerance 0.125 stopCheckEvery 7" in r.stdout, r.stdout


def test_a_bad_value_of_the_key_is_refused(tmp_path):
    build.build_host()
    _files(tmp_path, tol=-1.0)
    r = subprocess.run([build.TEST_STOP_TOLERANCE, str(tmp_path), "parse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "stopTolerance must be" in r.stderr, (r.returncode, r.stderr[-2000:])


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rapidnet.h")).read()
    declared = set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.load()
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    for method in ("apg_solve", "last_solve", "setStopTolerance", "stopTolerance"):
        assert hasattr(capi.Solver, method), method
    # every new entry point cites the member it extends, as its neighbours do
    for name in NEW:
        comment = hdr[: hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "SmpcController.cu:1500-1525" in comment and ":1480-1496" in comment, name


@pytest.mark.gpu
def test_stop_tolerance_keys_cpp(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = subprocess.run([build.TEST_STOP_TOLERANCE, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_stop_tolerance failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "stop tolerance: all checks passed" in r.stdout
