"""A re-weighted scenario tree through the C++ class surface (tests/cpp/test_tree_data.cpp): SmpcController::updateScenarioTree(path) between two
controlAction calls gives, bit for bit, the control of a fresh controller on the new files; ScenarioTree::reload of another topology throws and
changes nothing; Engine::setTreeDataDevice round-trips through getTreeData."""
import copy
import json
import os
import subprocess

import pytest

from rapidnet_amd import build, synth


def _files(tmp_path):
    from test_gpu_tree_data import reweighted

    p = synth.make_problem("tiny", max_iterations=40)
    old, new = os.path.join(str(tmp_path), "old"), os.path.join(str(tmp_path), "new")
    synth.write_problem(p, old)
    q = dict(p, tree=reweighted(p["tree"], synth.forecast_at(p["forecast"], 0), 7))
    synth.write_problem(q, new)
    bad = copy.deepcopy(p["tree"])
    bad["ancestor"][-1] -= 1                      # the last leaf hangs under its neighbour's parent: same counts, another topology
    path = os.path.join(str(tmp_path), "badTree.json")
    json.dump(bad, open(path, "w"))
    return old, new, path


def test_program_is_built_with_the_host_library():
    """compiles against the host headers and links: the new methods and the three C symbols exist"""
    build.build_host()
    assert os.path.exists(build.TEST_TREE_DATA)
    r = subprocess.run([build.TEST_TREE_DATA], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.gpu
def test_tree_data_cpp(tmp_path):
    build.build_host()
    r = subprocess.run([build.TEST_TREE_DATA, *_files(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "test_tree_data failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "tree data: all checks passed" in r.stdout
