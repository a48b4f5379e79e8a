"""No kernel of librapidnet_hip.so may spill, and every kernel has exactly one home.  hipcc's own resource report
(-Rpass-analysis=kernel-resource-usage) of every translation unit the library is built from must show 0 bytes of scratch per lane for
every kernel (round 4 shipped two that spilled: k_stream_gemv<float, NL, false, 2> and k_ls_eval); the host driver rapidnet_capi.hip
must compile NO kernel but its own k_sum_ranks -- everything it launches is declared `extern template` from the generated lists
(csrc/instantiations/*.inc) and compiled in one of the k_*.hip units: a kernel that the driver instantiates by itself means the lists are
out of date (python tools/gen_instantiations.py).  The chain walks also keep their occupancy: a change of the shared walk bodies (csrc/k_walks.hpp)
that costs a kernel a wave per SIMD -- a run-time guard in front of the first request once took k_down_chain<double, false> from 2 to 1 -- fails
here, before any run.  Cross-compiles for gfx950: no GPU needed."""
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

from rapidnet_amd import build


def _report(unit):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + [f for f in build.HIP_FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o",
                                                                              os.path.join(tmp, "k.o"), os.path.join(build.CSRC, unit + ".hip")]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, scratch = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur:
            OCCUPANCY[cur] = int(m.group(1))
    return scratch


OCCUPANCY = {}      # mangled kernel name -> waves per SIMD, filled by _report


def _occupancy_floor(name):
    """waves per SIMD that a chain walk (demangled name) had before its body was shared; None for every other kernel"""
    m = re.match(r"void rn::(k_down_chain_dual|k_down_chain|k_up_chain_cut|k_up_chain)<(double|float), (true|false)", name)
    if not m:
        return None
    kernel, fp64, flag = m.group(1), m.group(2) == "double", m.group(3) == "true"
    if kernel == "k_down_chain":      # flag: UNSC (no preconditioner entries requested)
        return 2 if fp64 else 4 if flag else 3
    if kernel == "k_down_chain_dual":
        return 2 if fp64 else 4
    if kernel == "k_up_chain":
        return 4 if fp64 else 5
    return 5


def test_no_kernel_uses_scratch_and_every_kernel_has_one_home():
    with ThreadPoolExecutor(max_workers=min(len(build.UNITS), os.cpu_count() or 4)) as ex:
        reports = dict(zip(build.UNITS, ex.map(_report, build.UNITS)))
    spilling = {k: v for r in reports.values() for k, v in r.items() if v > 0}
    assert not spilling, spilling
    driver = reports.pop("rapidnet_capi")
    assert all("k_sum_ranks" in k for k in driver) and len(driver) == 2, "rapidnet_capi.hip compiles kernels of its own (stale csrc/instantiations/*.inc?): %s" % sorted(driver)
    homes = {}
    for unit, r in reports.items():
        for k in r:
            assert k not in homes, "%s is compiled in %s and in %s" % (k, homes[k], unit)
            homes[k] = unit
    declared = sum(open(os.path.join(build.CSRC, "instantiations", f)).read().count("RN_LINKAGE template") for f in os.listdir(os.path.join(build.CSRC, "instantiations")))
    assert len(homes) == declared, (len(homes), declared)
    assert 150 < len(homes) < 200, "the resource reports list %d kernels" % len(homes)      # (round 5: 232)
    names = sorted(reports["k_walks"])
    demangled = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    floors = {k: _occupancy_floor(d) for k, d in zip(names, demangled)}
    walks = {k: f for k, f in floors.items() if f is not None}
    assert len(walks) == 4 + 6 + 4 + 8, sorted(walks)      # k_down_chain, k_down_chain_dual, k_up_chain, k_up_chain_cut
    below = {k: (OCCUPANCY[k], f) for k, f in walks.items() if OCCUPANCY[k] < f}
    assert not below, "chain walks below their occupancy floor (waves/SIMD, floor): %s" % below
