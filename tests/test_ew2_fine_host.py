"""The fine r^2-indexed Ewald table (64 intervals per octave of s = r^2, two degree-5 polynomials; k_culled EWK = 3) beside the
ordinary one (32 per octave, degree 6), both fetched through the host-only ``ceg_ew2_table`` (no GPU): the records evaluated in
float64 in the kernel's Horner order at 17 points per interval against mpmath.

Bound, per octave of s: the fine table's worst relative error -- over both functions of a record, B0 = erfc(alpha r)/r and
C = 2 alpha/sqrt(pi) exp(-alpha^2 s) -- is at most 3 x the ordinary table's on that octave + 2e-15.  Interpolation at Chebyshev
nodes gives a ratio of at most 2.3 for B0, which sets the worst error of either table on every octave; the remainder covers the
float64 rounding of the Horner chains, which dominates both tables below 16 A^2.  (C alone: degree 5 on half the width against
degree 6 has the error ratio 0.4375 / (alpha^2 h) with h the width of an ordinary interval, e.g. 3.4 for alpha = 0.35 on
[32, 64) A^2 -- 3.7e-14 against 1.1e-14, beside B0's 2.7e-13 there.  The figures of each function are printed.)

The 17 points of an interval are its 16 equal steps from the lower end and the last double below the upper end (the upper end itself
belongs to the next interval).  An ordinary interval is two fine ones, so its points are among the fine table's: one mpmath
reference per alpha, computed once at the fine points up to 12 A and shared by both tables and both cutoffs."""
import numpy as np
import pytest

from ceg_hip.plan import ew2_table

ALPHAS = (0.2, 0.26505830360350674, 0.35)
CUTOFFS = (9.0, 12.0)
R_EXACT2 = 4.0
LOGM = {False: 5, True: 6}
DEGREE = {False: 6, True: 5}


def _hi32(s: float) -> int:
    return int(np.array([s], dtype=np.float64).view(np.uint64)[0] >> np.uint64(32))


def _interval_points(base, ni, logm):
    """s[ni, 17] and the interval starts s_lo[ni]: keys base .. base + ni - 1 of a layout with 2^logm intervals per octave"""
    shift = 20 - logm
    keys = np.arange(base, base + ni + 1, dtype=np.uint64)
    edges = (keys << np.uint64(32 + shift)).view(np.float64)
    lo, hi = edges[:-1], edges[1:]
    s = lo[:, None] + (hi - lo)[:, None] * (np.arange(17) / 16.0)[None, :]
    s[:, 16] = np.nextafter(hi, 0.0)
    return s, lo


_REF = {}


def _reference(alpha, s):
    """{s: (B0, C)} in mpmath at 40 digits; values already known are not recomputed"""
    import mpmath
    mpmath.mp.dps = 40
    known = _REF.setdefault(alpha, {})
    a = mpmath.mpf(alpha)
    ka = 2 * a / mpmath.sqrt(mpmath.pi)
    for x in np.unique(s):
        x = float(x)
        if x not in known:
            m = mpmath.mpf(x)
            r = mpmath.sqrt(m)
            known[x] = (mpmath.erfc(a * r) / r, ka * mpmath.exp(-a * a * m))
    return known


def _errors(alpha, cutoff, fine):
    """(s[ni, 17], rel[2][ni, 17], ref[2][ni, 17], base, ni): the relative error of both functions at every point"""
    import mpmath
    tab, base, ni, worst, used = ew2_table(alpha, cutoff * cutoff, fine, R_EXACT2)
    assert tab is not None and tab.shape == (ni, 2 * (DEGREE[fine] + 1))
    assert used == (worst < 5e-11)          # (alpha = 0.35 at 12 A: neither fit holds a plan's tolerance, the table is judged all the same)
    s, lo = _interval_points(base, ni, LOGM[fine])
    t = s - lo[:, None]
    nd = DEGREE[fine] + 1
    ref = _reference(alpha, s)
    rel, val = [], []
    for f in range(2):
        co = tab[:, f * nd:(f + 1) * nd]
        v = np.broadcast_to(co[:, nd - 1:nd], t.shape).copy()
        for c in range(nd - 2, -1, -1):                  # the kernel's chain: v = fma(v, t, c_k), highest coefficient first
            v = v * t + co[:, c:c + 1]
        e = np.empty(s.shape)
        r = np.empty(s.shape)
        for idx in np.ndindex(s.shape):
            exact = ref[float(s[idx])][f]
            e[idx] = float(abs((mpmath.mpf(float(v[idx])) - exact) / exact))
            r[idx] = float(exact)
        rel.append(e)
        val.append(r)
    # what the builder reports is of the same size as what is found here (its points differ in the last one of each interval)
    assert max(e.max() for e in rel) < 2.0 * worst + 1e-14
    return s, rel, val, base, ni


@pytest.fixture(scope="module")
def errors():
    cache = {}

    def get(alpha, cutoff, fine):
        key = (alpha, cutoff, fine)
        if key not in cache:
            cache[key] = _errors(alpha, cutoff, fine)
        return cache[key]
    return get


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_fine_table_within_three_times_the_ordinary_one_per_octave(errors, alpha, cutoff):
    sc, rc, _, base_c, ni_c = errors(alpha, cutoff, False)
    sf, rf, _, base_f, ni_f = errors(alpha, cutoff, True)
    assert base_c == _hi32(R_EXACT2) >> 15 and base_f == _hi32(R_EXACT2) >> 14
    assert ni_f == 2 * ni_c and sf[-1, -1] == sc[-1, -1]     # the fine table covers the range of the ordinary one
    lo = R_EXACT2
    octaves = 0
    while lo < cutoff * cutoff:
        mc, mf = (sc >= lo) & (sc < 2.0 * lo), (sf >= lo) & (sf < 2.0 * lo)
        assert mc.any() and mf.any()
        for f, name in ((0, "B0"), (1, "C")):
            print(f"alpha {alpha} cutoff {cutoff} s in [{lo:g}, {2 * lo:g}) {name}: ordinary {rc[f][mc].max():.2e}  fine {rf[f][mf].max():.2e}")
        # the worst error of a table on the octave: over both functions of its records
        wc, wf = max(rc[f][mc].max() for f in range(2)), max(rf[f][mf].max() for f in range(2))
        assert wf <= 3.0 * wc + 2e-15, (alpha, cutoff, lo, wf, wc)
        lo *= 2.0
        octaves += 1
    assert octaves == (5 if cutoff == 9.0 else 6)


def test_fine_table_meets_the_single_pair_bounds(errors):
    """alpha of the CHA workload, 12 A: the bounds test_fast_math_accuracy_single_pair sets for the Coulomb columns -- 3e-11 of the
    local value, 1.5e-12 below 5.6 A, 5e-12 against a floor of 1 % of the column's largest magnitude -- hold for B0 and C of the fine
    table, the two values every Coulomb channel is formed from."""
    s, rel, ref, base, ni = errors(ALPHAS[1], 12.0, True)
    assert ni == 330 and base == _hi32(R_EXACT2) >> 14
    inside = s < 12.0 * 12.0
    for f in range(2):
        assert rel[f][inside].max() < 3e-11
        assert rel[f][s < 5.6 * 5.6].max() < 1.5e-12
        err = rel[f] * np.abs(ref[f])
        assert (err / np.maximum(np.abs(ref[f]), 1e-2 * np.abs(ref[f]).max()))[inside].max() < 5e-12


def test_layouts_and_limits():
    for alpha in ALPHAS:
        tab, base, ni, _, _ = ew2_table(alpha, 144.0, True)
        assert tab is not None and (ni, base) == (330, _hi32(R_EXACT2) >> 14) and tab.shape == (330, 12)
        tab, base, ni, _, _ = ew2_table(alpha, 144.0, False)
        assert tab is not None and (ni, base) == (165, _hi32(R_EXACT2) >> 15) and tab.shape == (165, 14)
    assert ew2_table(ALPHAS[1], 144.0, True)[4] and ew2_table(ALPHAS[1], 144.0, False)[4]
    # 21 A: 441 A^2 lies 216 ordinary / 432 fine intervals above 4 A^2 -- neither table (the plan keeps the erfcx variant)
    tab, base, ni, _, used = ew2_table(4.5 / 21.0, 441.0, True)
    assert tab is None and not used and ni == 432 and base == _hi32(R_EXACT2) >> 14
    tab, _, ni, _, used = ew2_table(4.5 / 21.0, 441.0, False)
    assert tab is None and not used and ni == 216
    # 14 A: the fine table would need 356 intervals, the ordinary one 178 of 176
    assert ew2_table(0.25, 196.0, True)[::2] == (None, 356, False) and ew2_table(0.25, 196.0, False)[::2] == (None, 178, False)
    # 13.5 A still has both (348 / 174 intervals)
    assert ew2_table(0.25, 13.5 * 13.5, True)[2] == 348 and ew2_table(0.25, 13.5 * 13.5, True)[4]
    assert ew2_table(0.25, 13.5 * 13.5, False)[2] == 174
    # a wider exact path moves the base
    tab, base, ni, _, used = ew2_table(0.25, 144.0, True, r_exact2=7.29)
    assert used and base == _hi32(7.29) >> 14 and ni < 330 and tab.shape == (ni, 12)
    # refused arguments yield no table
    assert ew2_table(0.0, 144.0, True)[::2] == (None, 0, False) and ew2_table(0.25, 3.0, True)[::2] == (None, 0, False)


def test_the_ordinary_table_is_memoised_beside_the_fine_one():
    """alternating requests return the same tables (one memo slot per layout)"""
    a = ew2_table(0.3, 100.0, False)[0]
    b = ew2_table(0.3, 100.0, True)[0]
    assert a.shape[1] == 14 and b.shape[1] == 12
    assert np.array_equal(a, ew2_table(0.3, 100.0, False)[0]) and np.array_equal(b, ew2_table(0.3, 100.0, True)[0])
