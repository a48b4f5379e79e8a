"""Cross-check of the JSON data formats against the REFERENCE's own loader classes (oracle/_ref/libref_loaders.so,
built by oracle/build_ref.sh from the reference's sources in place): the reference fixture AND the synthetic problem
files written by rapidnet_amd.synth must read back identically (to fp32, the reference parses with GetFloat()).

What the loaders read from each of these inputs is recorded under tests/golden/ref_loaders/<case>.npz (data only:
`python tests/test_ref_loaders.py --record` with the loaders built).  Every test checks the files as they are now against
that record; where oracle/_ref is built, the loaders also read the files live and must reproduce the record exactly.

The reference's ScenarioTree constructor writes past two of its heap blocks (it allocates N / N+1 entries for
nodesPerStage / nodesPerStageCumul but the JSON carries N+1 / N+2, ScenarioTree.cu:66-75), so its code is only ever
run in a CHILD process that leaves through os._exit(): `python tests/test_ref_loaders.py <directory> <out.npz>`, with a
heap-padding preload (oracle/malloc_pad.c, built by oracle/build_ref.sh) so that the overrun cannot reach a chunk header."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rapidnet_amd import synth  # noqa: E402
LIB = os.path.join(ROOT, "oracle", "_ref", "libref_loaders.so")
RECORDS = os.path.join(ROOT, "tests", "golden", "ref_loaders")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_fixture")
SYNTHETIC = ("toy", "small", "medium")
NET_ARRAYS = ("matA", "matB", "matGd", "matE", "matEd", "vecXmin", "vecXmax", "vecXsafe", "vecUmin", "vecUmax", "costAlpha1")
TREE_INTS = ("stages", "leaves", "children", "ancestor", "nChildren", "nChildrenCumul")
TREE_ARRAYS = ("probNode", "errorDemandNode", "errorPriceNode")
CONFIG_ARRAYS = ("matL", "matLhat", "costW", "matDiagPrecnd", "currentX", "prevU", "prevDemand")


def _lib():
    lib = C.CDLL(LIB)
    for f in ("ref_network_new", "ref_tree_new", "ref_config_new", "ref_forecaster_new"):
        getattr(lib, f).restype = C.c_void_p
        getattr(lib, f).argtypes = [C.c_char_p]
    for f in ("ref_network_array", "ref_tree_array", "ref_config_array"):
        getattr(lib, f).restype = C.POINTER(C.c_float)
        getattr(lib, f).argtypes = [C.c_void_p, C.c_char_p]
    lib.ref_tree_int_array.restype = C.POINTER(C.c_int)
    lib.ref_tree_int_array.argtypes = [C.c_void_p, C.c_char_p]
    lib.ref_config_string.restype = C.c_char_p
    lib.ref_config_string.argtypes = [C.c_void_p, C.c_char_p]
    for f in ("ref_network_dims", "ref_tree_dims", "ref_config_dims", "ref_forecaster_dims", "ref_config_scalars"):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p]
    lib.ref_forecaster_predict.argtypes = [C.c_void_p, C.c_int]
    for f in ("ref_forecaster_demand", "ref_forecaster_prices"):
        getattr(lib, f).restype = C.POINTER(C.c_float)
        getattr(lib, f).argtypes = [C.c_void_p]
    return lib


def _jsons(d):
    return [json.load(open(os.path.join(d, f))) for f in ("network.json", "scenarioTree.json", "controllerConfig.json", "forecastor.json")]


def _read_dir(d):
    """Everything the reference's loaders read from the four files of d, as arrays (runs the reference's code: child process only)."""
    lib = _lib()
    net, tree, cfg, fc = _jsons(d)
    dims = (C.c_int * 8)()
    got = {}

    def f32(ptr, n):
        return np.ctypeslib.as_array(ptr, shape=(n,)).copy()
    h = lib.ref_network_new(os.path.join(d, "network.json").encode())
    lib.ref_network_dims(h, dims)
    got["network.dims"] = np.array(dims[:4])
    for k in NET_ARRAYS:
        got["network." + k] = f32(lib.ref_network_array(h, k.encode()), np.size(net[k]))
    h = lib.ref_tree_new(os.path.join(d, "scenarioTree.json").encode())
    lib.ref_tree_dims(h, dims)
    got["tree.dims"] = np.array(dims[:5])
    for k in TREE_INTS:
        got["tree." + k] = np.ctypeslib.as_array(lib.ref_tree_int_array(h, k.encode()), shape=(len(tree[k]),)).copy()
    for k in TREE_ARRAYS:
        got["tree." + k] = f32(lib.ref_tree_array(h, k.encode()), np.size(tree[k]))
    h = lib.ref_config_new(os.path.join(d, "controllerConfig.json").encode())
    lib.ref_config_dims(h, dims)
    got["config.dims"] = np.array(dims[:5])
    sc = (C.c_float * 3)()
    lib.ref_config_scalars(h, sc)
    got["config.scalars"] = np.array(list(sc), np.float32)
    for k in CONFIG_ARRAYS:
        got["config." + k] = f32(lib.ref_config_array(h, k.encode()), np.size(cfg[k]))
    got["config.algorithmName"] = np.array(lib.ref_config_string(h, b"algorithmName").decode())
    h = lib.ref_forecaster_new(os.path.join(d, "forecastor.json").encode())
    lib.ref_forecaster_dims(h, dims)
    got["forecast.dims"] = np.array(dims[:4])
    keys = list(fc.keys())
    for t in range(2):
        got["forecast.predict%d" % t] = np.array(lib.ref_forecaster_predict(h, t))
        got["forecast.demand%d" % t] = f32(lib.ref_forecaster_demand(h), np.size(fc[keys[4 + 2 * t]]))
        got["forecast.prices%d" % t] = f32(lib.ref_forecaster_prices(h), np.size(fc[keys[5 + 2 * t]]))
    return got


def _close(got, expected):
    e = np.asarray(expected, float)
    return got.shape == (e.size,) and np.allclose(got.astype(float), e, rtol=2e-7, atol=1e-30)


def _check_dir(d, got):
    """what the reference's loaders read (`got`, live or recorded) against the four files of d"""
    net, tree, cfg, fc = _jsons(d)
    assert list(got["network.dims"]) == [net["nx"][0], net["nu"][0], net["nd"][0], net["ne"][0]]
    for k in NET_ARRAYS:
        assert _close(got["network." + k], net[k]), k
    assert list(got["tree.dims"]) == [tree["N"][0], tree["K"][0], tree["nodes"][0], tree["nNonLeafNodes"][0], tree["nChildrenTot"][0]]
    for k in TREE_INTS:
        assert np.array_equal(got["tree." + k], np.asarray(tree[k], int)), k
    for k in TREE_ARRAYS:
        assert _close(got["tree." + k], tree[k]), k
    assert list(got["config.dims"]) == [cfg["nx"][0], cfg["nu"][0], cfg["nd"][0], cfg["nv"][0], cfg["maxIterations"][0]]
    assert np.allclose(list(got["config.scalars"]), [cfg["stepSize"][0], cfg["penaltyStateX"][0], cfg["penaltySafetyX"][0]], rtol=2e-7)
    for k in CONFIG_ARRAYS:
        assert _close(got["config." + k], cfg[k]), k
    assert str(got["config.algorithmName"]) == cfg["algorithmName"]
    assert list(got["forecast.dims"]) == [fc["N"][0], fc["simHorizon"][0], fc["dimDemand"][0], fc["dimPrices"][0]]
    keys = list(fc.keys())
    for t in range(2):
        assert int(got["forecast.predict%d" % t]) == 1
        assert _close(got["forecast.demand%d" % t], fc[keys[4 + 2 * t]])
        assert _close(got["forecast.prices%d" % t], fc[keys[5 + 2 * t]])
        dh, ah = synth.forecast_at(fc, t)     # this repo's member-order rule is the reference's
        assert _close(got["forecast.demand%d" % t], dh) and _close(got["forecast.prices%d" % t], ah)


PAD = os.path.join(ROOT, "oracle", "_ref", "libmalloc_pad.so")


def _read_in_child(directory, out):
    # the child preloads oracle/malloc_pad.c: every heap request is padded, so the reference constructor's 4-byte overrun
    # (ScenarioTree.cu:66-75) lands in padding instead of the next chunk's header whatever the heap layout is
    env = dict(os.environ)
    if os.path.exists(PAD):
        env["LD_PRELOAD"] = PAD + (":" + env["LD_PRELOAD"] if env.get("LD_PRELOAD") else "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), directory, out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "REF_LOADERS_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _check(name, directory, tmp_path):
    """the files of `directory` against what the reference's loaders read from them when the record was made; with the loaders
    built, they read the files again in a child process and must reproduce the record exactly"""
    with np.load(os.path.join(RECORDS, name + ".npz")) as f:
        rec = dict(f)
    _check_dir(directory, rec)
    if os.path.exists(LIB):
        live = os.path.join(str(tmp_path), "live_%s.npz" % name)
        _read_in_child(directory, live)
        with np.load(live) as f:
            got = dict(f)
        assert sorted(got) == sorted(rec)
        for k in rec:
            assert got[k].dtype == rec[k].dtype and np.array_equal(got[k], rec[k]), k


def test_reference_fixture_through_reference_loaders(tmp_path):
    _check("reference_fixture", FIXTURE, tmp_path)


@pytest.mark.parametrize("name", SYNTHETIC)
def test_synthetic_files_through_reference_loaders(tmp_path, name):
    d = tmp_path / "files"
    synth.write_problem(synth.make_problem(name), str(d))
    _check(name, str(d), tmp_path)


def record():
    """tests/golden/ref_loaders/<case>.npz from the reference's loaders (oracle/_ref built)"""
    import tempfile

    os.makedirs(RECORDS, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        cases = [("reference_fixture", FIXTURE)]
        for name in SYNTHETIC:
            synth.write_problem(synth.make_problem(name), os.path.join(tmp, name))
            cases.append((name, os.path.join(tmp, name)))
        for name, d in cases:
            _read_in_child(d, os.path.join(RECORDS, name + ".npz"))
            print(name, os.path.getsize(os.path.join(RECORDS, name + ".npz")))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--record":
        record()
        sys.exit(0)
    got = _read_dir(sys.argv[1])
    _check_dir(sys.argv[1], got)
    np.savez_compressed(sys.argv[2], **got)
    print("REF_LOADERS_OK", flush=True)
    os._exit(0)   # skip interpreter teardown: the reference's loaders have corrupted the heap by now
