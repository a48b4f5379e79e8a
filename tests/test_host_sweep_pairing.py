"""The optional "sweepPairing" key of the controller configuration and Engine::setSweepPairing / getSweepPairing through the C++ class surface
(tests/cpp/test_sweep_pairing.cpp): "auto" for every file without the key, "on" / "off" where a file asks, anything else refused."""
import json
import os
import subprocess

import pytest

from rapidnet_amd import build, synth


def _files(tmp_path, bad=None):
    plain = synth.write_problem(synth.make_problem("small", max_iterations=40), str(tmp_path))
    cfg = json.load(open(plain))
    cfg["operatorMode"] = "dense"
    json.dump(cfg, open(plain, "w"))
    for name, value in (("On", "on"), ("Off", "off"), ("Auto", "auto")) + ((("Bad", bad),) if bad is not None else ()):
        cfg["sweepPairing"] = value
        json.dump(cfg, open(os.path.join(str(tmp_path), "controller%sConfig.json" % name), "w"))


def _run(mode, tmp_path, timeout=120):
    return subprocess.run([build.TEST_SWEEP_PAIRING, mode, str(tmp_path)], capture_output=True, text=True, timeout=timeout)


def test_program_is_built_with_the_host_library():
    build.build_host()
    assert os.path.exists(build.TEST_SWEEP_PAIRING)


@pytest.mark.parametrize("bad", ["yes", "ON", ""])
def test_the_key_parses_and_a_bad_value_is_refused(tmp_path, bad):
    """the loader needs no GPU: no key -> "auto", "auto" / "on" / "off" as written, any other string does not load"""
    build.build_host()
    _files(tmp_path, bad)
    r = _run("parse", tmp_path)
    assert "pairing keys: auto on off auto" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert r.returncode == 3 and "sweepPairing must be" in r.stderr and "CHECK failed" not in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.gpu
def test_engine_takes_the_key_and_its_accessor_round_trips(tmp_path):
    build.build_host()
    _files(tmp_path)
    r = _run("engine", tmp_path, timeout=600)
    assert r.returncode == 0 and "sweep pairing: all checks passed" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
