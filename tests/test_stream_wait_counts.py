"""The first requests of k_stream_gemv's walk go out back to back (csrc/k_stream.hpp, "THE WAIT COUNTS").

A chunk of the walk over half-spans requests its partial group (up to DU - 1 units, each under `if (d < nHead)`) and the first full group (DU units) before it
consumes anything.  The first version's ISA had an `s_waitcnt vmcnt(0)` in front of every one of those requests but the first -- the compiler could not pair a
conditional request with its conditional use and waited for everything in flight before it formed the next address -- so a block of about 20 live units paid
one memory round trip per unit of its head.  RN_LANDED (an s_waitcnt of the walk's own at points where nothing it names is in flight) keeps the compiler's counts
exact.  This test reads the gfx950 assembly of the three instantiations the 493-scenario tree runs (NL = 2, two workgroups per CU; DU = 8): the first
2 * DU - 1 = 15 block requests of the kernel have no wait on the vector-memory counter between them.  Cross-compiles: no GPU needed."""
import os
import re
import subprocess
import tempfile

import pytest

from rapidnet_amd import build

DU = 8      # units per group of k_stream_gemv<T, 2, true, 1, ST> (StreamDepth: 2 * (RN_STREAM_D - 1))
KERNELS = {"fp64": "_ZN2rn13k_stream_gemvIdLi2ELb1ELi1EdEE", "fp64 over fp32 blocks": "_ZN2rn13k_stream_gemvIdLi2ELb1ELi1EfEE", "fp32": "_ZN2rn13k_stream_gemvIfLi2ELb1ELi1EfEE"}


@pytest.fixture(scope="module")
def assembly():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k_stream.s")
        cmd = [build.HIPCC] + [f for f in build.HIP_FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", "-o", out, os.path.join(build.CSRC, "k_stream.hip")]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        return open(out).read().splitlines()


def body(lines, prefix):
    start = [i for i, l in enumerate(lines) if l.startswith(prefix) and l.rstrip().split(";")[0].rstrip().endswith(":")]
    assert len(start) == 1, (prefix, len(start))
    out = []
    for l in lines[start[0] + 1:]:
        out.append(l)
        if "s_endpgm" in l:
            return out
    raise AssertionError("no s_endpgm behind " + prefix)


@pytest.mark.parametrize("form", sorted(KERNELS))
def test_first_requests_of_a_chunk_are_issued_back_to_back(assembly, form):
    events = []
    for l in body(assembly, KERNELS[form]):
        if re.search(r"\bglobal_load_dwordx4\b.*\bnt\b", l):
            events.append("L")
        elif re.search(r"\bs_waitcnt\b.*\bvmcnt\(", l):
            events.append("w")
    seq = "".join(events)
    first = seq.find("L")
    assert first >= 0, "no non-temporal block request in the kernel"
    run = len(seq[first:]) - len(seq[first:].lstrip("L"))
    assert run >= 2 * DU - 1, "%s: only %d block requests before the first wait on vmcnt (%s...)" % (form, run, seq[first:first + 40])
