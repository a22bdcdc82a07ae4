"""Host side of the rotation-axis reduction of energy_grid (``ceg_energy_grid_reduced``): the mirror of the reference's
``meanBoltzmann`` (src/utils.jl:415-443) against an evaluation in 80-digit decimal arithmetic, the N-D branch against the 1-D
branch, and the compiled reduction kernel's resource usage.

Bound of the first test.  With f_k = w_k exp((m - x_k)/T) the mean is sum(f x)/sum(f).  A term that is not flushed to zero has
|(m - x)/T| <= 745, so the two roundings of that argument (the subtraction and the division; m itself cancels in the quotient)
move f by at most a few 745 * 2^-53 ~ 8e-14 relative; the host exp of an ulp and the two sums of at most 64 terms of one sign
of weight add less than 2e-14.  An error of relative size e in every f moves the mean by at most 2 e sum(f |x|)/sum(f), but
the part of e common to all terms cancels, and what remains is bounded here by 1e-13 sum(f |x|)/sum(f): the bound of the device
test (1e-12, tests/test_gpu_energy_grid_reduced.py) without its factor of ten for the device's exp and summation order."""
import re
import subprocess
from decimal import Decimal, getcontext
from pathlib import Path

import numpy as np
import pytest

from ceg_hip.hostmirror.utils import mean_boltzmann

ROOT = Path(__file__).resolve().parent.parent


def _exact(x, T, w):
    """-> (mean, sum(f |x|)/sum(f)) in 80-digit decimal arithmetic, f_k = w_k exp((min - x_k)/T): the shift of the formula is
    applied analytically (any shift cancels in the quotient).  Terms more than 2000 T above the minimum are left out: their
    share of either sum is below exp(-2000)."""
    getcontext().prec = 80
    xs = [Decimal(float(v)) for v in x]
    ws = [Decimal(1)] * len(xs) if w is None else [Decimal(float(v)) for v in w]
    Td, lo = Decimal(float(T)), min(xs)
    num = den = mag = Decimal(0)
    for v, wk in zip(xs, ws):
        arg = (lo - v) / Td
        if arg < -2000:
            continue
        f = arg.exp() * wk
        den += f
        num += f * v
        mag += f * abs(v)
    return num / den, mag / den


def _columns():
    rng = np.random.default_rng(415)
    big = 1e100
    return {
        "ordinary negative energies": -rng.uniform(200.0, 4000.0, 50),
        "mixed signs": rng.uniform(-1500.0, 2500.0, 40),
        "one dominant minimum": np.concatenate([[-9000.0], rng.uniform(-100.0, 100.0, 30)]),
        "all equal": np.full(17, -1234.5678),
        "all equal, zero": np.zeros(5),
        "some 1e100": np.concatenate([rng.uniform(-3000.0, 500.0, 9), [big, big, big]])[rng.permutation(12)],
        "all 1e100": np.full(7, big),
        "a single element": np.array([-321.0]),
        "spread beyond the underflow point": np.array([-50000.0, -49990.0, 0.0, 1e6, 3.0e5, -49000.0]),
        "64 entries": rng.normal(-800.0, 600.0, 64),
    }


@pytest.mark.parametrize("T", [77.0, 300.0, 1000.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_mean_boltzmann_against_decimal_arithmetic(T, weighted):
    rng = np.random.default_rng(7)
    worst = 0.0
    for name, col in _columns().items():
        w = rng.uniform(0.01, 3.0, len(col)) if weighted else None
        ref, scale = _exact(col, T, w)
        bound = 1e-13 * float(scale)
        # 1-D branch
        got = mean_boltzmann(col, T, w)
        err = abs(Decimal(got) - ref)
        worst = max(worst, float(err) / bound if bound else float(err))
        assert err <= Decimal(bound), (name, "1-D", got, float(ref), float(err) / bound if bound else float(err))
        # N-D branch: the column at one position of a 4-D array among unrelated columns
        A = rng.uniform(-2000.0, 2000.0, (len(col), 3, 2, 2))
        A[:, 1, 0, 1] = col
        got4 = mean_boltzmann(A, T, w)
        assert got4.shape == (3, 2, 2)
        err4 = abs(Decimal(float(got4[1, 0, 1])) - ref)
        assert err4 <= Decimal(bound), (name, "4-D", got4[1, 0, 1], float(ref))
        if name == "all 1e100":
            assert got >= 1e90 and got4[1, 0, 1] >= 1e90
        if name == "some 1e100":
            assert got < 1e4                                   # blocked orientations drop out of the mean
    print(f"  T = {T}, weighted = {weighted}: worst error / bound = {worst:.3g}")


def test_nd_branch_equals_the_columnwise_1d_call_bit_for_bit():
    """The reference's own use (output_cube, compute_levels): meanBoltzmann(grid, T) on an Array{Float64,4}."""
    rng = np.random.default_rng(842)
    A = rng.uniform(-4000.0, 1000.0, (11, 4, 3, 5))
    A[rng.uniform(size=A.shape) < 0.2] = 1e100
    A[:, 0, 0, 0] = 1e100
    A[:, 1, 1, 1] = -77.0
    w = rng.uniform(0.1, 2.0, 11)
    for T in (77.0, 300.0):
        for weights in (None, w):
            B = mean_boltzmann(A, T, weights)
            assert B.shape == A.shape[1:] and B.dtype == np.float64
            for i in np.ndindex(*B.shape):
                one = mean_boltzmann(A[(slice(None),) + i], T, weights)
                assert isinstance(one, float)
                assert np.float64(one).view(np.int64) == B[i].view(np.int64), (T, i, one, B[i])
    assert mean_boltzmann(A, 300.0)[0, 0, 0] >= 1e90


def test_nan_element_makes_the_mean_nan():
    col = np.array([-100.0, np.nan, -300.0])
    assert np.isnan(mean_boltzmann(col, 300.0))
    assert np.isnan(mean_boltzmann(col[:, None], 300.0)[0])


def test_abi_constant_matches_the_header():
    from ceg_hip import _abi
    m = re.search(r"#define\s+CEG_EGRID_MAX_TEMPS\s+(\d+)", (ROOT / "include" / "ceg_hip.h").read_text())
    assert m and int(m.group(1)) == _abi.EGRID_MAX_TEMPS == 8


def test_reduction_kernel_uses_no_scratch(tmp_path):
    """Compile-time guard (hipcc cross-compiles without a GPU): every variant of k_egrid_reduce (one per number of temperatures)
    keeps its partial sums in registers -- 0 bytes of scratch per lane, no spilled registers, no LDS."""
    hipcc = Path("/opt/rocm/bin/hipcc")
    if not hipcc.exists():
        pytest.skip("no hipcc")
    csrc = ROOT / "crystalenergygrids.jl_amd" / "csrc"
    flags = re.search(r"CXXFLAGS\s*=\s*(.*?)\nSRCS", (csrc / "Makefile").read_text(), re.S).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    r = subprocess.run([str(hipcc), *flags, "-c", "--cuda-device-only", "-o", str(tmp_path / "egrid.o"), "ceg_egrid.hip",
                        "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    mine = [b for b in blocks if "k_egrid_reduce" in b.splitlines()[0]]
    assert len(mine) == 9, [b.splitlines()[0] for b in blocks]                     # 0 .. CEG_EGRID_MAX_TEMPS temperatures

    def field(block, name):
        return int(re.search(name + r": (\d+)", block).group(1))
    for b in mine:
        occupancy = field(b, r"Occupancy \[waves/SIMD\]")
        print(f"  {b.splitlines()[0].split()[0]}: VGPRs {field(b, 'VGPRs')}, occupancy {occupancy}")
        assert field(b, "ScratchSize [^:]*") == 0
        assert field(b, "VGPRs Spill") == 0 and field(b, "SGPRs Spill") == 0
        assert field(b, "LDS Size [^:]*") == 0
        assert occupancy >= 4
