"""The host code behind rn_shift_warm_start / rn_get_shift_map (rapidnet_amd/csrc/shift_map.hpp, plain C++: the node correspondence of the
shifted warm start) under AddressSanitizer and UBSan on the CPU, as a stand-alone program (tests/cpp/shift_map_sanitize.cpp), and against
the numpy restatement (tests/shift_oracle.py) on 300 random ragged trees plus the suite's hand-made ones."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import shift_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_tree(rng):
    """(parent, nodesPerStageCumul): 1 .. 8 stages, every node above the last stage with 1 .. 4 children"""
    N = int(rng.integers(1, 9))
    parent, cum, stage_nodes = [-1], [0, 1], [0]
    for _ in range(1, N):
        nxt = []
        for i in stage_nodes:
            for _ in range(int(rng.integers(1, 5))):
                nxt.append(len(parent))
                parent.append(i)
        stage_nodes = nxt
        cum.append(len(parent))
    return np.array(parent), np.array(cum)


def cases():
    from rapidnet_amd import synth

    rng = np.random.default_rng(20)
    out = []
    for _ in range(300):
        parent, cum = random_tree(rng)
        nc = int((parent == 0).sum())
        out.append((parent, cum, int(rng.integers(0, max(nc, 1)))))
    for name in ("late", "horizon1", "ragged", "fan"):
        tree = synth.make_problem(name)["tree"]
        parent, _ = so.tree_arrays(tree)
        cum = np.asarray(tree["nodesPerStageCumul"], int).ravel()[: int(tree["N"][0]) + 1]
        for child in range(max(int((parent == 0).sum()), 1)):
            out.append((parent, cum, child))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_shift_map_is_clean_under_asan_and_ubsan_and_is_the_restatements(tmp_path):
    exe = str(tmp_path / "shift_map_sanitize")
    src = os.path.join(ROOT, "tests", "cpp", "shift_map_sanitize.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src], check=True, timeout=600)
    trees = cases()
    path = str(tmp_path / "trees.txt")
    with open(path, "w") as f:
        f.write("%d\n" % len(trees))
        for parent, cum, child in trees:
            f.write("%d %d %d\n%s\n%s\n" % (len(parent), len(cum) - 1, child, " ".join(map(str, parent)), " ".join(map(str, cum))))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "shift map runs %d" % len(trees) and len(lines) == len(trees) + 1
    shapes = set()
    for (parent, cum, child), line in zip(trees, lines):
        got = np.array(line.split(), int)
        assert np.array_equal(got, so.shift_map(parent, child)), (parent.tolist(), child)
        shapes.add((len(cum) - 1, int((parent == 0).sum())))
    assert len(shapes) > 20      # the random trees differ in depth and in the root's fan-out
