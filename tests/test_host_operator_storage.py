"""The optional "operatorStorage" key of the controller configuration through the C++ class surface (tests/cpp/test_operator_storage.cpp):
fp32 operator blocks under fp64 iterates for a controller whose file asks for them, the engine's own element type for every other file."""
import json
import os
import subprocess

import pytest

from rapidnet_amd import build, synth


def _files(tmp_path):
    plain = synth.write_problem(synth.make_problem("small", max_iterations=40), str(tmp_path))
    cfg = json.load(open(plain))
    cfg["operatorMode"] = "dense"
    json.dump(cfg, open(plain, "w"))
    cfg["operatorStorage"] = "f32"
    json.dump(cfg, open(os.path.join(str(tmp_path), "controllerF32Config.json"), "w"))


def test_program_is_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_OPERATOR_STORAGE)


def test_a_bad_value_of_the_key_is_refused(tmp_path):
    """the loader needs no GPU: a configuration whose key holds anything but "native" or "f32" does not load"""
    build.build_host()
    _files(tmp_path)
    bad = os.path.join(str(tmp_path), "controllerF32Config.json")
    cfg = json.load(open(bad))
    cfg["operatorStorage"] = "f16"
    json.dump(cfg, open(bad, "w"))
    r = subprocess.run([build.TEST_OPERATOR_STORAGE, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "operatorStorage must be" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.gpu
def test_operator_storage_key_cpp(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = subprocess.run([build.TEST_OPERATOR_STORAGE, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_operator_storage failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "storage: f32 config -> f32, plain config -> native" in r.stdout and "operator storage: all checks passed" in r.stdout
