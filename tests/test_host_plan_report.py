"""The plan report (rn_plan_report, rn_plan_report_scenarios, rn_plan_report_device) through the layers that need no GPU: the entry points in
the header, in the library's exports and in the Python binding, each citing the reference members it generalises; null contexts refused at
the boundary; the host classes' members.  On a GPU the program tests/cpp/test_plan_report.cpp runs a control step through
SmpcController, and this file reads what it wrote: controlAction(fstream&)'s own output is unchanged byte for byte and the "planReport"
entry is a JSON object that holds the program's figures."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rapidnet_amd import build, capi, synth

NEW = ("rn_plan_report", "rn_plan_report_scenarios", "rn_plan_report_device")
RN_E_ARG = -1


def test_program_is_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_PLAN_REPORT)


def test_new_symbols_are_declared_exported_bound_and_cited():
    hdr = open(os.path.join(ROOT, "include", "rapidnet.h")).read()
    declared = set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.load()
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    comment = hdr[: hdr.index("int rn_plan_report(")].rsplit("/* Plan report", 1)[1]
    assert "updateKpi" in comment and "getEconomicKpi" in comment and "SmpcController.cu:1819-1859" in comment
    cols = re.search(r"enum \{ (RN_PLAN_ECON[^}]*)\}", hdr).group(1)
    names = re.findall(r"RN_PLAN_[A-Z_]+", cols)
    assert names == ["RN_PLAN_ECON", "RN_PLAN_SMOOTH", "RN_PLAN_STORED", "RN_PLAN_SHORT_EXP", "RN_PLAN_XBOX_EXP", "RN_PLAN_UBOX_EXP", "RN_PLAN_SHORT_MAX",
                     "RN_PLAN_XBOX_MAX", "RN_PLAN_UBOX_MAX", "RN_PLAN_COLS"]
    assert len(capi.PLAN_COLUMNS) == len(names) - 1 and capi.PLAN_SUMS == names.index("RN_PLAN_SHORT_MAX")
    for method in ("planReport", "planReportDevice", "planLeaves"):
        assert hasattr(capi.Solver, method), method
    for cls, member in (("Engine.hpp", "evaluatePlan"), ("Engine.hpp", "PlanReport"), ("SmpcController.hpp", "getPlanReport"), ("SmpcController.hpp", "writePlanReport")):
        assert member in open(os.path.join(ROOT, "rapidnet_amd", "csrc", "host", cls)).read(), (cls, member)
    inc = open(os.path.join(ROOT, "rapidnet_amd", "csrc", "plan_report.inc")).read()
    assert "SmpcController.cu:1819-1859" in inc and "updateKpi" in inc


def test_null_contexts_are_refused_without_a_gpu():
    """(wrong counts, NULL outputs and the state rules need a live context, hence a device: tests/test_gpu_plan_report.py)"""
    lib = capi.load()
    out, ln = np.full(9, 7.0), np.full(1, 7, np.int32)
    a, b, n = C.c_void_p(5), C.c_void_p(5), C.c_size_t(5)
    assert lib.rn_plan_report(None, 1, out.ctypes.data) == RN_E_ARG
    assert lib.rn_plan_report_scenarios(None, 1, out.ctypes.data, ln.ctypes.data) == RN_E_ARG
    assert lib.rn_plan_report_device(None, C.byref(a), C.byref(b), C.byref(n)) == RN_E_ARG
    assert (out == 7.0).all() and ln[0] == 7 and (a.value, b.value, n.value) == (5, 5, 5)


@pytest.mark.gpu
def test_plan_report_cpp(tmp_path):
    build.build_host()
    synth.write_problem(synth.make_problem("small", max_iterations=60), str(tmp_path))
    r = subprocess.run([build.TEST_PLAN_REPORT, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_plan_report failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "plan report: all checks passed" in r.stdout
    plain = open(os.path.join(str(tmp_path), "plain.json")).read()
    lines = open(os.path.join(str(tmp_path), "report.json")).read().splitlines(keepends=True)
    assert plain == lines[0] and plain.startswith('"control" : [')         # controlAction(fstream&)'s own output, byte for byte
    assert lines[1].startswith('"planReport" : {') and lines[2].startswith('"control" : [') and len(lines) == 3
    doc = json.loads("{" + lines[1] + "}")["planReport"]
    stages, scenarios = (int(v) for v in re.search(r"shape: (\d+) stages, (\d+) scenarios", r.stdout).groups())
    assert doc["columns"] == list(capi.PLAN_COLUMNS)
    st, sc = np.array(doc["perStage"]), np.array(doc["perScenario"])
    assert st.shape == (stages, 9) and sc.shape == (scenarios, 9) and len(doc["leafNode"]) == scenarios
    econ, stored = (float(v) for v in re.search(r"stage0: econ (\S+) stored (\S+)", r.stdout).groups())
    assert st[0, 0] == econ and st[0, 2] == stored                          # 17 significant digits: the doubles themselves
    assert np.isfinite(st).all() and np.isfinite(sc).all() and (st[:, 2] > 0).all()
