"""The solve certificate (rn_solve_certificate, rn_solve_certificate_device) through the layers that need no GPU: the entry points in the
header, in the library's exports and in the Python binding, each marked as an extension with the reference lines it builds on; null contexts
refused at the boundary; the host classes' members.  On a GPU the program tests/cpp/test_certificate.cpp runs control steps through
SmpcController on `small` and `medium`, dense and structured, and this file reads what it wrote: controlAction(fstream&)'s own output is
unchanged byte for byte and the "solveCertificate" entry is a JSON object with named fields that holds the program's figures."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rapidnet_amd import build, capi, synth

NEW = ("rn_solve_certificate", "rn_solve_certificate_device")
RN_E_ARG = -1


def test_program_is_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_CERTIFICATE)


def test_new_symbols_are_declared_exported_bound_and_cited():
    hdr = open(os.path.join(ROOT, "include", "rapidnet.h")).read()
    declared = set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.load()
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    comment = hdr[: hdr.index("int rn_solve_certificate(")].rsplit("/* ---- the solve certificate", 1)[1]
    assert "Extension" in comment and "solveStep" in comment and "proximalFunG" in comment and "computeValueFbe" in comment
    assert "VALID = 1" in comment and "U_EXCESS = 0" in comment and "rn_algorithmic_bytes" in comment
    cols = re.search(r"enum \{ (RN_CERT_DUAL[^}]*)\}", hdr).group(1)
    names = re.findall(r"RN_CERT_[A-Z_]+", cols)
    assert names == ["RN_CERT_DUAL", "RN_CERT_PRIMAL", "RN_CERT_GAP", "RN_CERT_COST", "RN_CERT_INNER", "RN_CERT_SUPPORT", "RN_CERT_DIST_X", "RN_CERT_DIST_S",
                     "RN_CERT_U_EXCESS", "RN_CERT_NORM_X", "RN_CERT_NORM_S", "RN_CERT_XIS_POS", "RN_CERT_ABS_TERMS", "RN_CERT_VALID", "RN_CERT_COLS"]
    assert re.search(r"RN_CERT_COLS = 16", cols) and capi.CERT_COLS == 16 and len(capi.CERT_COLUMNS) == len(names) - 1
    bufs = re.search(r"enum rn_buffer \{(.*?)\}", hdr, re.S) or re.search(r"RN_BUF_X = 0(.*?)RN_BUF_COUNT", hdr, re.S)
    ids = re.findall(r"\bRN_BUF_[A-Z_]+", re.sub(r"/\*.*?\*/", "", bufs.group(0), flags=re.S))
    assert ids[-3:] == ["RN_BUF_CERT_X", "RN_BUF_CERT_U", "RN_BUF_COUNT"]          # appended in front of RN_BUF_COUNT
    assert (capi.BUF_CERT_X, capi.BUF_CERT_U) == (ids.index("RN_BUF_CERT_X"), ids.index("RN_BUF_CERT_U"))
    for method in ("solveCertificate", "solveCertificateDevice"):
        assert hasattr(capi.Solver, method), method
    for cls, member in (("Engine.hpp", "solveCertificate"), ("SmpcController.hpp", "getSolveCertificate"), ("SmpcController.hpp", "writeSolveCertificate")):
        assert member in open(os.path.join(ROOT, "rapidnet_amd", "csrc", "host", cls)).read(), (cls, member)
    inc = open(os.path.join(ROOT, "rapidnet_amd", "csrc", "certificate.inc")).read()
    assert "SmpcController.cu:563-755" in inc and "Extension" in inc


def test_null_contexts_are_refused_without_a_gpu():
    """(NULL outputs and the state rules need a live context, hence a device: tests/test_gpu_certificate.py)"""
    lib = capi.load()
    out, a = np.full(capi.CERT_COLS, 7.0), C.c_void_p(5)
    assert lib.rn_solve_certificate(None, out.ctypes.data) == RN_E_ARG
    assert lib.rn_solve_certificate_device(None, C.byref(a)) == RN_E_ARG
    assert (out == 7.0).all() and a.value == 5


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", ["small", "medium"])
def test_certificate_cpp(tmp_path, name, mode):
    build.build_host()
    p = synth.make_problem(name, max_iterations=60)
    p["config"] = dict(p["config"], operatorMode=mode)
    synth.write_problem(p, str(tmp_path))
    r = subprocess.run([build.TEST_CERTIFICATE, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_certificate failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "solve certificate: all checks passed" in r.stdout
    plain = open(os.path.join(str(tmp_path), "plain.json")).read()
    lines = open(os.path.join(str(tmp_path), "certificate.json")).read().splitlines(keepends=True)
    assert plain == lines[0] and plain.startswith('"control" : [')         # controlAction(fstream&)'s own output, byte for byte
    assert lines[1].startswith('"solveCertificate" : {') and lines[2].startswith('"control" : [') and len(lines) == 3
    doc = json.loads("{" + lines[1] + "}")["solveCertificate"]
    assert list(doc) == list(capi.CERT_COLUMNS)
    dual, primal, uexc, valid = (float(v) for v in re.search(r"record: dual (\S+) primal (\S+) uExcess (\S+) valid (\S+)", r.stdout).groups())
    assert (doc["dual"], doc["primal"], doc["uExcess"], doc["valid"]) == (dual, primal, uexc, valid)      # 17 significant digits: the doubles themselves
    assert all(np.isfinite(v) for v in doc.values()) and doc["gap"] == doc["primal"] - doc["dual"]
