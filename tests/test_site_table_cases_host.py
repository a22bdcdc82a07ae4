"""``tests/site_table_cases.py`` checked on the CPU, so that ``tests/test_gpu_site_table_shapes.py`` cannot pass vacuously: the claims
about the drawn sites, the longdouble reference against the oracle's pair sums and against ``recip_cases.reference`` of one- and
two-molecule systems, the derived bounds against a float64 NumPy evaluation, and the tile and launch arithmetic restated by hand."""
import re
from pathlib import Path

import numpy as np
import pytest

import interp_cases as IC
import pair_rule_cases as PR
import recip_cases as RC
import site_table_cases as S

LD = np.longdouble
SOURCE = Path(__file__).resolve().parent.parent / "crystalenergygrids.jl_amd" / "csrc"
PLACED = [c.name for c in S.CASES if c.family != "thresholds" and not c.refused]
FLOAT64_WORST = {}


# ------------------------------------------------------------------------------------------------ the case table
def test_restated_constants_and_lines_are_those_of_the_source():
    state = (SOURCE / "ceg_mc_state.h").read_text()
    assert re.search(r"constexpr int MC_THREADS = (\d+);", state).group(1) == str(S.MC_THREADS)
    assert re.search(r"constexpr int MC_MAX_ATOMS = (\d+);", state).group(1) == "16" == str(max(S.MOLECULE_M))
    site = (SOURCE / "ceg_site.hip").read_text()
    assert "const int nk = h->v.nk, n_pad = (n + 15) & ~15, tiles = n_pad / 16;" in site
    assert "if (ti > tj) return;" in site and "for (int kc = 0; kc < nk; kc += 4)" in site
    assert "for (int64_t q = tid; q < v.nk; q += MC_THREADS)" in site
    assert "tables_bytes(h, m_atoms) > 64 * 1024" in site


def test_every_claimed_shape_is_in_the_table():
    by = {}
    for c in S.CASES:
        by.setdefault(c.family, []).append(c)
    assert [c.n for c in by["edges"]] == [1, 2, 15, 16, 17, 31, 32, 33, 48, 49] and all(c.m == 3 and c.k.nk == 114 for c in by["edges"])
    assert S.kinds_of(3).tolist() == [0, 1, 0] and sorted(set(S.kinds_of(5).tolist())) == [0, 1, 2, 3]
    assert [(c.n, c.m) for c in by["tiles17"]] == [(257, 3)]
    assert [c.m for c in by["molecule"]] == [1, 2, 5, 8, 16] and all(c.n == 33 for c in by["molecule"])
    assert [c.k.nk for c in by["kloop"]] == [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 316] and all((c.n, c.m) == (17, 3) for c in by["kloop"])
    for c in by["kloop"]:
        k = c.k
        if k.nk:
            assert k.kf[0] == 20.0 and (k.nk == 1 or k.kf[1:].max() <= 1.0)
            assert (k.ijk[:, 0] >= 0).all() and len({tuple(v) for v in k.ijk}) == k.nk                  # from the half space, no repeats
    assert {c.name for c in by["terms"]} == {"terms-zero-charges", "terms-empty-rules", "terms-no-grids"} and all(c.n == 33 for c in by["terms"])
    assert not S.BY_NAME["terms-zero-charges"].q.any() and S.table("empty").nrules == 0
    # the LDS limit: 16 bytes per (atom, table entry)
    ok, bad = S.BY_NAME["lds-stride256"], S.BY_NAME["lds-stride257"]
    assert ok.k.stride == 256 and 16 * ok.m * ok.k.stride == 64 * 1024 and bad.k.stride == 257 and bad.refused and ok.m == bad.m == 16
    kx, ky, kz = (int(x) for x in ok.k.ks)
    assert {kx} <= set(ok.k.ijk[:, 0].tolist()) and {ky, -ky} <= set(ok.k.ijk[:, 1].tolist()) and {kz, -kz} <= set(ok.k.ijk[:, 2].tolist())
    tri = S.BY_NAME["triangular-n33"]
    assert np.array_equal(np.triu(tri.mat), tri.mat) and (tri.n, tri.m, tri.k.nk) == (33, 3, 114)
    gen = S.CELLS["general"]
    assert (np.abs(gen) > 1e-2).all() and (np.abs(np.linalg.inv(gen)) > 1e-4).all()
    # charges: three distinct non-zero ones and a zero; grids: one kind without
    assert sorted(S.CHARGES).count(0.0) == 1 and len(set(S.CHARGES)) == 4
    vdw, coul, _inside = S.grid_set()
    assert [g is None for g in vdw] == [False, False, False, True] and coul is not None
    assert len({g.csetup.npoints for g in vdw[:3]}) == 3
    assert S.OFFSET_ONE == 2.0 * S.ENC + S.STATIC and S.OFFSET_ONE != 0.0 and S.OFFSET_PAIR != 0.0


def test_rule_table_gives_every_pair_of_kinds_an_entry_of_its_own():
    t = S.table("full")
    nk = t.nkinds
    assert nk == 4 and len(t.offsets) == nk * nk + 1
    names = {}
    for a in range(nk):
        for b in range(nk):
            lo, hi = t.offsets[a * nk + b], t.offsets[a * nk + b + 1]
            assert hi > lo, (a, b)                                                                   # every pair has an entry
            assert t.entry_of[a][b] == t.entry_of[b][a]
            lo2, hi2 = t.offsets[b * nk + a], t.offsets[b * nk + a + 1]
            assert t.rules[lo:hi].tobytes() == t.rules[lo2:hi2].tobytes()                             # symmetric
            names[(min(a, b), max(a, b))] = t.entry_name(t.entry_of[a][b])
    assert len(set(names.values())) == 10                                                           # depends on both kinds
    assert {"LJ", "LJ+CED", "Buckingham", "CED", "HS+Buckingham+CED"} <= set(names.values())
    assert sum(1 for v in names.values() if v.startswith("HS")) == 1 and t.spheres(t.entry_of[0][0]) == [S.SPHERE]
    # a repeated kind index (kinds[aj] for both) reaches another entry for every mixed pair of the molecule (0, 1, 0)
    assert t.entry_of[1][1] != t.entry_of[1][0] != t.entry_of[0][0]


@pytest.mark.parametrize("n", sorted({c.n for c in S.CASES}))
def test_tile_and_launch_arithmetic(n):
    n_pad, tiles, writers = S.launch_shape(n)
    assert n_pad % 16 == 0 and 0 <= n_pad - n <= 15 and tiles == -(-n // 16)
    assert len(writers) == tiles * (tiles + 1) // 2 and all(ti <= tj for ti, tj in writers)
    # every pair i < j lies in exactly one writing tile; the tiles below the diagonal hold no such pair
    I, J = np.triu_indices(n, 1)
    assert set(zip((I // 16).tolist(), (J // 16).tolist())) | {(t, t) for t in range(tiles)} == set(writers)
    by_hand = {1: (16, 1), 2: (16, 1), 15: (16, 1), 16: (16, 1), 17: (32, 2), 21: (32, 2), 31: (32, 2), 32: (32, 2), 33: (48, 3), 48: (48, 3),
               49: (64, 4), 257: (272, 17)}
    assert (n_pad, tiles) == by_hand[n]


def test_padding_of_15_and_the_257_subset():
    assert S.launch_shape(257)[0] - 257 == 15 and S.launch_shape(17)[0] - 17 == 15 and S.launch_shape(33)[0] - 33 == 15
    c = S.BY_NAME["tiles17"]
    I, J = S.compared_pairs(c)
    have = set(zip(I.tolist(), J.tolist()))
    assert (I < J).all() and len(have) == len(I) < 257 * 256 // 2
    for a in list(range(17)) + list(range(240, 257)):
        assert all((min(a, b), max(a, b)) in have for b in range(257) if b != a), a
    for t in range(16, 257, 16):
        for b in range(t - 15, t + 16):
            if b < 257:
                assert b == 40 or (min(40, b), max(40, b)) in have
                assert b == 200 or (min(200, b), max(200, b)) in have
    assert {(i // 16, j // 16) for i, j in have} >= {(0, t) for t in range(17)} | {(t, 16) for t in range(16)}          # (tile (16, 16) holds site 256 alone)
    assert len(have) >= 34 * 257 + 256


# ------------------------------------------------------------------------------------------------ the sites
@pytest.mark.parametrize("name", PLACED)
def test_site_placement_claims(name):
    c = S.BY_NAME[name]
    e = S.expected(name)
    pos, n = e.pos, c.n
    assert pos.shape == (n, c.m, 3) and np.isfinite(pos).all()
    frac = pos.reshape(-1, 3) @ c.inv.T
    if n >= 3:
        # the 27-image shortcut is not enough: atoms tens of A outside the cell, more than one lattice vector away
        outside = np.abs(pos.reshape(-1, 3)).max(axis=1)
        assert outside.max() > 60.0 and (np.abs(np.floor(frac)) >= 2).any()
    r2min = e.r2.reshape(len(e.I), c.m * c.m).min(axis=1)
    cut2 = S.CUTOFF ** 2
    pair = {(int(i), int(j)): q for q, (i, j) in enumerate(zip(e.I, e.J))}
    if n >= 15:
        assert (r2min >= cut2).any(), "no pair with every atom pair beyond the cutoff"
    if n >= 3:
        # sites 0 and 2: within the cutoff only across cell faces
        direct = min(np.linalg.norm(p - q) for p in pos[0] for q in pos[2])
        assert r2min[pair[(0, 2)]] < cut2 and direct > 60.0
    if n >= 2:
        assert r2min[pair[(0, 1)]] < cut2
    # hard spheres
    hard = e.hard
    sphere_kinds = c.table == "full"
    k0 = np.nonzero(c.kinds == 0)[0]
    overlap = (e.r2[:, k0][:, :, k0].reshape(len(e.I), len(k0) ** 2) < S.SPHERE ** 2).any(axis=1) if sphere_kinds else np.zeros(len(e.I), dtype=bool)
    assert np.array_equal(hard, overlap)
    if sphere_kinds and n >= 4:
        assert hard[pair[(0, 3)]] and hard.sum() >= 1
    if sphere_kinds and n >= 15:
        assert hard.sum() <= 0.05 * len(hard), (hard.sum(), len(hard))
    elif sphere_kinds:
        assert hard.sum() <= 1
    # margins from the thresholds
    for t in (cut2, S.SPHERE ** 2):
        assert (np.abs(e.r2 - t) > 1e-9 * t).all(), t
    # exactly one blocked site (site 4), where the grids are used
    assert e.blocked.tolist() == [c.grids and i == 4 for i in range(n)]
    if c.grids:
        free = ~e.blocked
        assert (np.abs(e.grid[free]) > 0).all() and (e.grid_T[free] > 0).all()
    # every term is live where it is meant to be
    soft = ~hard
    if c.k.nk and c.charges == "mixed":
        assert (np.abs(e.R) > 0).all() and (np.abs(e.recip - S.OFFSET_ONE) > 0).all()
    else:
        assert not e.R.any() and (e.recip == LD(S.OFFSET_ONE)).all() and not e.R_tol.any()
    if c.table == "empty":
        assert not e.P.any() and not e.P_size.any()
    elif n >= 15:
        assert (np.abs(e.P[soft]) > 1.0).sum() >= 4


def test_threshold_case_places_pairs_on_both_sides():
    c = S.BY_NAME["thresholds"]
    pos = S.sites(c.name)
    sat = np.arange(1, c.n)
    r2 = S.pair_r2(c, pos, np.zeros(len(sat), dtype=np.int64), sat)[:, 0, 0]
    want = np.array([t * (1.0 + d) for t in (S.CUTOFF ** 2, S.SPHERE ** 2) for d in S.THRESHOLD_DELTAS for _ in range(2)])
    assert (np.abs(r2 - want) <= 1e-13 * want).all()                              # placed to within rounding of the target
    for t, rows in ((S.CUTOFF ** 2, r2[:10]), (S.SPHERE ** 2, r2[10:])):
        assert (rows < t).any() and (rows >= t).any() and (np.abs(rows - t) <= 2e-12 * t).all()
    exp = S.threshold_expected(c)
    vals = set(exp[np.triu_indices(c.n, 1)].tolist())
    assert vals == {np.inf, -1.75 + S.OFFSET_PAIR, S.OFFSET_PAIR}
    assert (0.9 + 0.6) ** 2 == S.SPHERE ** 2


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", ["edges-n17", "molecule-m5", "triangular-n33"])
def test_pair_sums_against_the_oracle(oracle, name):
    """P_ij against the oracle's single_contribution_vdw (float64, energy.jl:407-427): site j alone in the box, site i on trial"""
    c = S.BY_NAME[name]
    e = S.expected(name)
    t = S.table(c.table)
    worst = 0.0
    for j in range(c.n):
        sel = np.nonzero(e.J == j)[0]
        if not len(sel):
            continue
        got = oracle.single_contribution_vdw_raw(c.mat, c.inv, *t.args(), e.pos[j], c.kinds, np.zeros(c.m, dtype=np.int32), e.pos[e.I[sel]], c.kinds, -1)
        hard = e.hard[sel]
        assert not (got[hard] < 1e90).any()
        err = np.abs(got[~hard].astype(LD) - e.P[sel][~hard])
        tol = LD(1e-9) * e.P_size[sel][~hard]
        assert (err <= tol).all(), (name, j)
        worst = max(worst, float((err / np.where(tol > 0, tol, LD(1))).max()) if len(err) else 0.0)
    print(f"{name}: oracle float64 pair sums within {worst:.3g} of the P tolerance")


@pytest.mark.parametrize("name", ["edges-n17", "molecule-m16", "kloop-nk5", "triangular-n33"])
def test_reciprocal_terms_against_two_molecule_systems(name):
    """recip[i] + recip[j] + R_ij - offsets = the reciprocal energy of the two-molecule system as ``recip_cases.reference`` gives it for
    one molecule of 2 m atoms (sitehopping.jl:41-82 telescoped); and ``structure_factors`` is the S that reference forms"""
    c = S.BY_NAME[name]
    e = S.expected(name)
    k = c.k
    again = S.recip_from_sf(k, e.sre, e.sim)
    T = RC.magnitude(k.kf, k.sf, c.q, S.ENC, S.STATIC)
    assert (np.abs(again - e.recip) <= LD(2.0) ** -58 * T).all()
    rng = np.random.default_rng(3)
    sel = rng.choice(len(e.I), min(40, len(e.I)), replace=False)
    both = np.concatenate([e.pos[e.I[sel]], e.pos[e.J[sel]]], axis=1)
    two = RC.reference(c.inv, k.ijk, k.kf, k.sf, np.concatenate([c.q, c.q]), both, 0.0, 0.0)
    one = e.recip - LD(S.OFFSET_ONE)
    want = two - one[e.I[sel]] - one[e.J[sel]]
    T2 = RC.magnitude(k.kf, k.sf, np.concatenate([c.q, c.q]), 0.0, 0.0)
    assert (np.abs(want - e.R[sel]) <= LD(2.0) ** -56 * T2).all()


def test_grid_terms_are_those_of_the_host_mirror():
    """v0 + v1 against ceg_hip.grids.interpolate_grid (float64, the reference's COEFF X form) atom by atom"""
    from ceg_hip import grids as G
    c = S.BY_NAME["molecule-m5"]
    e = S.expected(c.name)
    vdw, coul, _inside = S.grid_set()
    for i in np.nonzero(~e.blocked)[0][:12]:
        total = 0.0
        for a, kind in enumerate(c.kinds):
            if vdw[kind] is not None:
                total += G.interpolate_grid(vdw[kind], e.pos[i, a])
            total += S.CHARGES[kind] * G.interpolate_grid(coul, e.pos[i, a])
        assert abs(LD(total) - e.grid[i]) <= IC.bound(e.grid_T[i]), i
    blocked = int(np.nonzero(e.blocked)[0][0])
    assert G.interpolate_grid(vdw[0], e.pos[blocked, 0]) == 1e100


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize("name", PLACED)
def test_float64_numpy_stays_inside_the_derived_bounds(name):
    c = S.BY_NAME[name]
    e = S.expected(name)
    rec64, R64 = S.float64_evaluation(e)
    err = np.abs(rec64.astype(LD) - e.recip)
    assert (err <= e.recip_tol).all()
    r1 = S._ratio(err, e.recip_tol)
    join = 4.0 * S.U * S.pair_magnitude(c)
    errR = np.abs(R64.astype(LD) - e.R)
    assert (errR <= e.R_tol).all()
    r2 = S._ratio(errR, e.R_tol)
    FLOAT64_WORST[name] = (r1, r2)
    print(f"{name}: float64 NumPy within {r1:.4f} of recip_bound, {r2:.4f} of pair_recip_bound (join {join:.3g})")
    # the whole tolerance through compare(): the float64 terms joined in float64, P and the grid terms rounded from the reference
    fw = np.where(e.blocked, 1e100, np.asarray(e.grid, dtype=np.float64) + rec64)
    it = np.full((c.n, c.n), np.nan)
    vals = (np.asarray(e.P, dtype=np.float64) + R64) + S.OFFSET_PAIR
    it[e.I, e.J] = it[e.J, e.I] = vals
    np.fill_diagonal(it, 1e100)
    if c.n > 64:                                                  # the elements outside the subset: anything symmetric
        it[np.isnan(it)] = 0.0
    S.compare(e, fw, rec64, it)


def test_compare_rejects_what_the_mutations_would_return():
    """the checker itself: each arithmetic slip of the kernels, applied to the reference, is outside the tolerance"""
    c = S.BY_NAME["edges-n17"]
    e = S.expected(c.name)

    def tables(R=None, P=None, recip=None):
        R = e.R if R is None else R
        rec = np.asarray(e.recip if recip is None else recip, dtype=np.float64)
        fw = np.where(e.blocked, 1e100, np.asarray(e.grid + (e.recip if recip is None else recip), dtype=np.float64))
        it = np.full((c.n, c.n), 1e100)
        it[e.I, e.J] = it[e.J, e.I] = np.asarray(((e.P if P is None else P) + R) + LD(S.OFFSET_PAIR), dtype=np.float64)
        return fw, rec, it
    S.compare(e, *tables())
    with pytest.raises(AssertionError, match="interactions"):
        S.compare(e, *tables(R=e.R / 2))                                               # the factor 2 of w dropped
    re_only = S.pair_recip_from_sf(c.k, e.sre, np.zeros_like(e.sim), e.I, e.J) * 2
    with pytest.raises(AssertionError, match="interactions"):
        S.compare(e, *tables(R=re_only))                                               # b.x in both MFMA calls ~ the real parts twice
    sre, sim = S.structure_factors(c.inv, c.k, np.ones(c.m), e.pos)
    with pytest.raises(AssertionError, match="recip"):
        S.compare(e, *tables(recip=S.recip_from_sf(c.k, sre, sim)))                      # s_q[a] omitted in molecule_sf
    kinds = c.kinds
    t = S.table("full")
    P = np.zeros(len(e.I), dtype=LD)
    for ai in range(c.m):
        for aj in range(c.m):
            P = P + PR.entry_energy_ld(t, t.entry_of[int(kinds[aj])][int(kinds[aj])], e.r2[:, ai, aj])[0]
    with pytest.raises(AssertionError):
        S.compare(e, *tables(P=P))                                                     # kinds[aj] for both kinds
