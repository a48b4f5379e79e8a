"""The plan bands (rn_plan_quantiles, rn_plan_quantiles_device, rn_plan_paths) through the layers that need no GPU: the entry points in the
header, in the library's exports and in the Python binding; null contexts refused at the boundary; the host-side checks of the cap on a
stage's width and of the levels, in a stand-alone host program (tests/cpp/test_bands_host.cpp) -- a 4097-wide stage is refused there and is
never built on a device; the host classes' members.  On a GPU the program tests/cpp/test_plan_bands.cpp runs a control step through
SmpcController, and this file reads what it wrote: controlAction(fstream&)'s own output is unchanged byte for byte and the "planBands" entry
is a JSON object that holds the program's figures."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rapidnet_amd import build, capi, synth

NEW = ("rn_plan_quantiles", "rn_plan_quantiles_device", "rn_plan_paths")
RN_E_ARG = -1


def test_programs_are_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_PLAN_BANDS) and os.path.exists(build.TEST_BANDS_HOST)


def test_width_cap_and_level_order_on_the_host():
    build.build_host()
    r = subprocess.run([build.TEST_BANDS_HOST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "bands host: all checks passed" in r.stdout, r.stdout


def test_new_symbols_are_declared_exported_bound_and_described():
    hdr = open(os.path.join(ROOT, "include", "rapidnet.h")).read()
    declared = set(re.findall(r"\b(rn_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.load()
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    comment = hdr[: hdr.index("int rn_plan_quantiles(")].rsplit("/* Plan bands", 1)[1]
    assert "no counterpart" in comment and "c_j >= q * c_m" in comment and "RN_E_STATE" in comment and "4096" in comment
    assert re.search(r"enum \{ RN_BAND_X = 0, RN_BAND_U = 1 \}", hdr) and (capi.BAND_X, capi.BAND_U) == (0, 1)
    assert int(re.search(r"RN_BAND_MAX_LEVELS = (\d+)", hdr).group(1)) == capi.BAND_MAX_LEVELS
    host = open(os.path.join(ROOT, "rapidnet_amd", "csrc", "bands_host.hpp")).read()
    assert int(re.search(r"MAX_LEVELS = (\d+)", host).group(1)) == capi.BAND_MAX_LEVELS and int(re.search(r"MAX_WIDTH = (\d+)", host).group(1)) == 4096
    for method in ("planQuantiles", "planQuantilesDevice", "planPaths", "bandLeaves"):
        assert hasattr(capi.Solver, method), method
    for cls, member in (("Engine.hpp", "planQuantiles"), ("Engine.hpp", "planPaths"), ("SmpcController.hpp", "getPlanBands"), ("SmpcController.hpp", "writePlanBands")):
        assert member in open(os.path.join(ROOT, "rapidnet_amd", "csrc", "host", cls)).read(), (cls, member)


def test_null_contexts_are_refused_without_a_gpu():
    """(wrong counts, levels, NULL outputs and the state rules need a live context, hence a device: tests/test_gpu_plan_bands.py)"""
    lib = capi.load()
    q, out, ln = np.array([0.5]), np.full(4, 7.0), np.full(1, 7, np.int32)
    a = C.c_void_p(5)
    assert lib.rn_plan_quantiles(None, capi.BAND_X, 1, q.ctypes.data, 1, out.ctypes.data) == RN_E_ARG
    assert lib.rn_plan_quantiles_device(None, capi.BAND_U, 1, q.ctypes.data, C.byref(a)) == RN_E_ARG
    assert lib.rn_plan_paths(None, capi.BAND_X, 1, out.ctypes.data, ln.ctypes.data) == RN_E_ARG
    assert (out == 7.0).all() and ln[0] == 7 and a.value == 5


@pytest.mark.gpu
def test_plan_bands_cpp(tmp_path):
    build.build_host()
    synth.write_problem(synth.make_problem("small", max_iterations=60), str(tmp_path))
    r = subprocess.run([build.TEST_PLAN_BANDS, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_plan_bands failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "plan bands: all checks passed" in r.stdout
    plain = open(os.path.join(str(tmp_path), "plain.json")).read()
    lines = open(os.path.join(str(tmp_path), "bands.json")).read().splitlines(keepends=True)
    assert plain == lines[0] and plain.startswith('"control" : [')          # controlAction(fstream&)'s own output, byte for byte
    assert lines[1].startswith('"planBands" : {') and lines[2].startswith('"control" : [') and len(lines) == 3
    doc = json.loads("{" + lines[1] + "}")["planBands"]
    N, L, nx, nu = (int(v) for v in re.search(r"shape: (\d+) stages, (\d+) scenarios, (\d+) nx, (\d+) nu", r.stdout).groups())
    assert doc["shape"] == [N, L, nx, nu, 3] and doc["levels"] == [0.05, 0.5, 0.95] and len(doc["leafNode"]) == L
    qx, qu = np.array(doc["xQuantiles"]).reshape(N, nx, 3), np.array(doc["uQuantiles"]).reshape(N, nu, 3)
    px, pu = np.array(doc["xPaths"]).reshape(L, N, nx), np.array(doc["uPaths"]).reshape(L, N, nu)
    mx, mu = (float(v) for v in re.search(r"median: x (\S+) u (\S+)", r.stdout).groups())
    assert qx[N - 1, 0, 1] == mx and qu[N - 1, 0, 1] == mu                   # 17 significant digits: the doubles themselves
    assert np.isfinite(qx).all() and np.isfinite(qu).all() and (np.diff(qx, axis=2) >= 0).all() and (np.diff(qu, axis=2) >= 0).all()
    # every band holds some path's value and lies within the paths' range at its stage
    assert (qx >= px.min(axis=0)[:, :, None]).all() and (qx <= px.max(axis=0)[:, :, None]).all()
    assert (qu >= pu.min(axis=0)[:, :, None]).all() and (qu <= pu.max(axis=0)[:, :, None]).all()
    assert np.isin(qx[N - 1], px[:, N - 1, :]).all()
