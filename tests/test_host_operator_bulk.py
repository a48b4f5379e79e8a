"""All per-node operator blocks in one call through the C++ class surface (tests/cpp/test_operator_bulk.cpp): Engine::setOperators /
getOperators on host arrays and setOperatorsDevice / getOperatorsDevice on device arrays round-trip bit for bit against the per-node
setOperator / getOperator, under native and under fp32 block storage."""
import json
import os
import subprocess

import pytest

from rapidnet_amd import build, synth


def _files(tmp_path):
    plain = synth.write_problem(synth.make_problem("tiny", max_iterations=40), str(tmp_path))
    cfg = json.load(open(plain))
    cfg["operatorMode"] = "dense"
    json.dump(cfg, open(plain, "w"))
    cfg["operatorStorage"] = "f32"
    json.dump(cfg, open(os.path.join(str(tmp_path), "controllerF32Config.json"), "w"))


def test_program_is_built_with_the_host_library():
    """compiles against Engine.hpp and links: the four methods and the four C symbols exist"""
    build.build_host()
    assert os.path.exists(build.TEST_OPERATOR_BULK)
    r = subprocess.run([build.TEST_OPERATOR_BULK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.gpu
def test_operator_bulk_cpp(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = subprocess.run([build.TEST_OPERATOR_BULK, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_operator_bulk failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "operator bulk: all checks passed" in r.stdout
