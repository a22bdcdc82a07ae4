"""``tests/pair_rule_cases.py`` checked on the CPU with the oracle alone, so that ``tests/test_gpu_pair_rules.py`` cannot pass
vacuously: the tables hold what they are meant to hold and would be routed where they are meant to go, the generated placements
really lie on both sides of every switch point, the crowd really overfills the hit queues, and the checker (the oracle's rule
energies) agrees with an independent longdouble restatement of the eight formulas."""
import ctypes as C

import numpy as np
import pytest

from ceg_hip import _abi
from ceg_hip.hostmirror.interactions import FF

import pair_rule_cases as PC

_CACHE = {}


def _refs(oracle, name, which="triangular"):
    """[(case, oracle energies, literal r^2)] of a table, computed once"""
    key = (name, which)
    if key not in _CACHE:
        t, mat = PC.table(name), PC.cell(which)
        inv = np.linalg.inv(mat)
        out = []
        for c in PC.single_pairs(t, mat):
            ref = oracle.single_contribution_vdw_raw(mat, inv, *t.args(), c.atom[None], [c.kind], [0], c.trial, [0], -1)
            out.append((c, ref, PC.literal_r2(mat, inv, c.atom, c.trial)))
        _CACHE[key] = out
    return _CACHE[key]


def test_every_kind_occurs_and_the_undefined_one_is_refused():
    seen = set()
    for name in PC.TABLES:
        t = PC.table(name)
        seen |= {int(k) for k in t.rules[:t.nrules]["kind"]}
        assert any(r["shift"] != 0.0 for r in t.rules[:t.nrules])
        for e in range(len(t.entries)):
            rules = t.entry_rules(e)
            assert not rules or any(s != 0.0 for _k, _p, s in rules), t.entry_name(e)
        # symmetric, and only row / column 0 filled (except in `wide`)
        off = t.offsets
        for a in range(t.nkinds):
            for b in range(t.nkinds):
                ra = t.rules[off[a * t.nkinds + b]:off[a * t.nkinds + b + 1]]
                rb = t.rules[off[b * t.nkinds + a]:off[b * t.nkinds + a + 1]]
                assert ra.tobytes() == rb.tobytes()
                if a and b and name != "wide":
                    assert len(ra) == 0
    assert seen == {int(k) for k in FF} - {int(FF.UndefinedInteraction)}
    bad = PC.rejected_table()
    assert {int(k) for k in bad.rules["kind"]} == {int(FF.UndefinedInteraction)}
    # refused on the host, before a device is looked for
    lib = _abi.load_library()
    mat = PC.cell("triangular")
    matT = np.ascontiguousarray(mat.T.reshape(9))
    invT = np.ascontiguousarray(np.linalg.inv(mat).T.reshape(9))
    h = C.c_void_p()
    assert lib.ceg_pairs_create(C.byref(h), 0, _abi.dptr(matT), _abi.dptr(invT), 144.0, bad.rules.ctypes.data, _abi.i32ptr(bad.offsets), 1,
                                PC.COULOMBIC) == -4
    assert not h.value
    charge = np.zeros(1)
    assert lib.ceg_mc_create(C.byref(h), 0, None, None, _abi.dptr(charge), 1, _abi.dptr(matT), _abi.dptr(invT), 144.0, bad.rules.ctypes.data,
                             _abi.i32ptr(bad.offsets), PC.COULOMBIC, None, None, None, None, 0, None, None) == -4
    assert not h.value


def test_alpha0_tables_are_one_table_in_two_orders():
    a, b = PC.table("alpha0_first"), PC.table("alpha0_last")
    assert [n for n, _r in a.entries] == [n for n, _r in b.entries]
    assert a.entry_name(a.entry_of_kind[0]) == PC.ALPHA0 and b.entry_name(b.entry_of_kind[-1]) == PC.ALPHA0
    # first / last CoulombEwaldDirect rule of the rule array is the one with alpha = 0
    ced = lambda t: [float(r["p"][0]) for r in t.rules[:t.nrules] if int(r["kind"]) == int(FF.CoulombEwaldDirect)]
    assert ced(a)[0] == 0.0 and all(x == PC.ALPHA for x in ced(a)[1:])
    assert ced(b)[-1] == 0.0 and ced(b)[0] == PC.ALPHA
    assert PC.ALPHA0 not in [n for n, _r in PC.table("fast").entries]


@pytest.mark.parametrize("name", PC.TABLES)
def test_predicted_path(name):
    t = PC.table(name)
    p = PC.predicted(t)
    assert (p["fast"], p["erfc"], p["pairs_lds"], p["mc_lds"]) == PC.INTENDED[name], p
    if name == "wide":
        assert p["bytes"] > 48 * 1024 and t.nkinds == 36
    if name == "short":
        assert t.cutoff ** 2 <= 1.0
    if name == "steep":
        assert any(int(r["kind"]) == int(FF.Exponential) and abs(r["p"][1] * t.cutoff - 701.0) < 1e-9 for r in t.rules[:t.nrules])
    if name == "edge_fast":
        assert 4.98 < max(r["p"][0] for r in t.rules[:t.nrules] if int(r["kind"]) == int(FF.CoulombEwaldDirect)) * t.cutoff < 5.0 * (1 - 1e-9)
    if name == "edge_slow":
        assert min(r["p"][0] for r in t.rules[:t.nrules] if int(r["kind"]) == int(FF.CoulombEwaldDirect)) * t.cutoff > 5.0


def test_table_edges():
    edges = PC.table_edges()
    assert len(edges) >= 40
    for s in edges:
        bits = np.array([s]).view(np.uint64)[0]
        assert int(bits) & ((1 << 47) - 1) == 0 and 1.0 < s < 144.0
    assert edges[0] == 1.0 + 1.0 / 32.0 and edges[-1] == 140.0               # the first interval's upper end, the last one's lower end
    assert {int(np.floor(np.log2(s))) for s in edges} == set(range(8))       # every octave of [1, 144]


@pytest.mark.parametrize("name", PC.TABLES)
def test_single_pairs_finite_share_and_spheres(oracle, name):
    t = PC.table(name)
    per_entry = {}
    for c, ref, r2 in _refs(oracle, name):
        assert not np.isnan(ref).any()
        inside = r2 < t.cutoff ** 2
        blocked = np.zeros(len(r2), dtype=bool)
        for s in t.spheres(c.entry):
            blocked |= inside & (r2 < s * s)
        assert np.array_equal(np.isinf(ref), blocked), (name, t.entry_name(c.entry))       # Inf: exactly the spheres, from within
        assert np.all(ref[blocked] == np.inf)
        f, n = per_entry.get(c.entry, (0, 0))
        per_entry[c.entry] = (f + int(np.isfinite(ref).sum()), n + len(ref))
    assert len(per_entry) == len(t.entries)
    for e, (f, n) in per_entry.items():
        assert f >= n / 3, (name, t.entry_name(e), f, n)
    assert 10000 <= sum(n for _f, n in per_entry.values()) <= 30000


@pytest.mark.parametrize("which", ["triangular", "rotated"])
def test_placements_straddle_every_switch_point(oracle, which):
    """the literal r^2 (the one the reference's rules are given) of the generated placements on both sides of 0.25, of 1.0, of each
    sampled interval edge and of each sphere radius; literal_r2 itself is pinned bit for bit by the plain-Coulomb entry, whose
    energy is two correctly rounded operations on r^2"""
    name = "fast"
    t = PC.table(name)
    below, above = {}, {}
    for c, ref, r2 in _refs(oracle, name, which):
        if t.entry_name(c.entry) == "Coulomb":
            kind, p, shift = t.entry_rules(c.entry)[0]
            want = np.where(r2 < t.cutoff ** 2, PC.COULOMBIC * p[0] * p[1] / np.sqrt(r2) - shift, 0.0)
            assert np.array_equal(ref, want)
        for tag in (PC.TAG_QUARTER, PC.TAG_ONE, PC.TAG_EDGE, PC.TAG_SPHERE):
            sel = c.tag == tag
            for s in np.unique(c.target[sel]):
                m = sel & (c.target == s)
                assert np.all(np.abs(r2[m] / s - 1.0) < 2.1e-6)
                below[(tag, s)] = below.get((tag, s), 0) + int((r2[m] < s).sum())
                above[(tag, s)] = above.get((tag, s), 0) + int((r2[m] >= s).sum())
                tight = m & (np.abs(c.delta) <= 1e-14)
                if tag != PC.TAG_EDGE:
                    assert np.all(np.abs(r2[tight] / s - 1.0) < 1e-12)                   # the tight ones are tight
        lo = c.tag == PC.TAG_LOG
        assert r2[lo].min() < 0.06 ** 2 and r2[lo].max() > (0.99 * t.cutoff) ** 2 and r2[lo].max() < t.cutoff ** 2
    keys = set(below)
    assert {k[0] for k in keys} == {PC.TAG_QUARTER, PC.TAG_ONE, PC.TAG_EDGE, PC.TAG_SPHERE}
    assert {s for g, s in keys if g == PC.TAG_EDGE} == set(PC.table_edges())
    assert {s for g, s in keys if g == PC.TAG_SPHERE} == {PC.SPHERE ** 2, PC.SPHERE_ALONE ** 2}
    for k in keys:
        assert below[k] >= 3 and above[k] >= 3, (k, below[k], above[k])


@pytest.mark.parametrize("name", ["fast", "edge_slow", "wide"])
def test_crowd_overfills_the_queues(oracle, name):
    t, mat = PC.table(name), PC.cell("triangular")
    inv = np.linalg.inv(mat)
    cr = PC.crowd(t, mat)
    assert len(cr.pos) == 600 and set(cr.kinds.tolist()) == set(range(t.nkinds))
    d = cr.pos[:, None, :] - cr.pos[None, :, :]
    d2 = np.sum(d * d, axis=2) + 1e9 * np.eye(len(cr.pos))
    assert d2.min() >= 1.2 ** 2
    near_one = near_quarter = total = 0
    fewest = 10 ** 9
    for m in PC.CROWD_SIZES:
        trial = cr.trials[m]
        for p in range(len(trial)):
            r2 = np.concatenate([PC.literal_r2(mat, inv, cr.pos, np.broadcast_to(trial[p, a], cr.pos.shape)) for a in range(m)])
            fewest = min(fewest, int((r2 < t.cutoff ** 2).sum()))
            assert int((r2 < t.cutoff ** 2).sum()) >= 128 + 64, (m, p)              # well over two batches: the two-at-a-time loop runs
            near_one += bool((r2 < 1.0).any())
            near_quarter += bool((r2 < 0.25).any())
            total += 1
        ref = oracle.single_contribution_vdw_raw(mat, inv, *t.args(), cr.pos, cr.kinds, cr.mol, trial, [0] * m, -1)
        assert not np.isnan(ref).any() and np.isfinite(ref).sum() >= len(ref) / 3 and np.isinf(ref).any()
    print(f"{name}: fewest pairs inside the cutoff {fewest}, r2 < 1 in {near_one} and r2 < 0.25 in {near_quarter} of {total} placements")
    assert near_one >= 0.1 * total and near_quarter >= 0.03 * total
    if name != "wide":                                     # the state's own pair sum is finite (ceg_mc_baseline is checked on it)
        per_mol = PC.crowd_pair_sums(oracle, t, mat, cr)
        assert np.isfinite(per_mol).all() and np.abs(per_mol).sum() > 0.0


@pytest.mark.parametrize("name", ["fast", "edge_slow", "alpha0_first", "two_alphas", "steep", "short"])
def test_oracle_rule_energies_against_longdouble(oracle, name):
    """the eight rule formulas restated in numpy longdouble (math.erfc of the oracle's own float64 argument for the two erfc kinds)
    agree with the oracle to 1e-13 of the sum of the absolute values of the entry's terms and shifts, on the whole single-pair set.
    `steep` alone (B cutoff = 701) is given the rounding of the exponential's float64 argument on top: 2^-52 B r of that term."""
    t = PC.table(name)
    worst = 0.0
    for c, ref, r2 in _refs(oracle, name):
        want, size = PC.entry_energy_ld(t, c.entry, r2)
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(want.astype(np.float64))), (name, t.entry_name(c.entry))
        err = np.abs(ref[fin].astype(PC.LD) - want[fin])
        tol = PC.LD(1e-13) * size[fin]
        if name == "steep":          # exp(-B r) with B r up to 701: the float64 roundings of the argument alone exceed 1e-13 of the term
            tol = tol + PC.LD(2.0 ** -52) * PC.exp_argument_size(t, c.entry, r2)[fin]
        ok = err <= tol
        assert ok.all(), (name, t.entry_name(c.entry), float(np.max(err / np.maximum(size[fin], PC.LD(1e-300)))))
        if (size[fin] > 0).any():
            worst = max(worst, float(np.max(err[size[fin] > 0] / size[fin][size[fin] > 0])))
    print(f"{name}: oracle vs longdouble, worst {worst:.2e} of the terms")
