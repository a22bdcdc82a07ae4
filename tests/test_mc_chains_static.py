"""Register budgets of the Monte-Carlo trial / accept kernels once their bodies are shared with the chain-group kernels
(k_mcg_trial / k_mcg_accept, ceg_mc_group.hip).  hipcc cross-compiles both files for gfx950 with the resource-usage remark; no GPU needed.

The batch-1 path sits at the edge of three waves per SIMD (168 VGPRs), so the refactoring must leave the existing kernels'
code as it was: the same VGPR counts and scratch, variant by variant.  The group variants may cost at most 8 VGPRs more
than their single-handle counterparts and no more scratch."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "crystalenergygrids.jl_amd" / "csrc"
HIPCC = Path("/opt/rocm/bin/hipcc")

# (FAST, INSERT, CELLS) -> (VGPRs, scratch bytes per lane) of k_mc_trial
TRIAL = {(1, 1, 1): (167, 12), (0, 1, 1): (159, 0), (1, 0, 1): (167, 12), (0, 0, 1): (159, 0),
         (1, 1, 0): (161, 0), (0, 1, 0): (151, 0), (1, 0, 0): (162, 0), (0, 0, 0): (152, 0)}
ACCEPT = (96, 0)


@pytest.fixture(scope="module")
def usage():
    if not HIPCC.exists():
        pytest.fail("hipcc is needed to check the kernel budgets")
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fvisibility=hidden", "-Dceg_EXPORTS"]
    out = {}
    name = None
    lines = []
    for source in ("ceg_mc.hip", "ceg_mc_group.hip"):        # k_mc_trial / k_mc_accept, then k_mcg_trial / k_mcg_accept
        r = subprocess.run([str(HIPCC), *flags, "--cuda-device-only", "-c", "-o", "/dev/null", source, "-Rpass-analysis=kernel-resource-usage"],
                           cwd=CSRC, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        lines += r.stderr.splitlines()
    for line in lines:
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark: *(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split()[0]] = int(m.group(2))
    return out


def _trial(usage, kernel, key):
    mangled = [n for n in usage if f"{kernel}ILb{key[0]}ELb{key[1]}ELb{key[2]}E" in n]
    assert len(mangled) == 1, (kernel, key, mangled)
    u = usage[mangled[0]]
    return u["VGPRs"], u["ScratchSize"], u["Occupancy"]


def test_existing_trial_and_accept_kernels_keep_their_code(usage):
    for key, (vgpr, scratch) in TRIAL.items():
        got = _trial(usage, "10k_mc_trial", key)
        assert got[:2] == (vgpr, scratch), (key, got)
        assert got[2] == 3, (key, got)
    acc = [n for n in usage if "11k_mc_acceptE" in n]
    assert len(acc) == 1
    assert (usage[acc[0]]["VGPRs"], usage[acc[0]]["ScratchSize"]) == ACCEPT


def test_group_kernels_stay_within_budget(usage):
    for key, (vgpr, scratch) in TRIAL.items():
        got = _trial(usage, "11k_mcg_trial", key)
        assert got[0] <= vgpr + 8 and got[1] <= scratch, (key, got, vgpr, scratch)
        assert got[2] == 3, (key, got)            # three waves per SIMD like the batch-1 kernel
    acc = [n for n in usage if "12k_mcg_acceptE" in n]
    assert len(acc) == 1
    assert usage[acc[0]]["VGPRs"] <= ACCEPT[0] + 8 and usage[acc[0]]["ScratchSize"] <= ACCEPT[1]
