"""The guest-guest pair arithmetic (energy.jl:397-427) of every kernel that evaluates it, over every rule kind
and every switch of the arithmetic, ONE PAIR PER OUTPUT: the cases of tests/pair_rule_cases.py (checked on the CPU by
tests/test_pair_rule_cases_host.py) against oracle_single_contribution_vdw.  Run with `pytest -m gpu` on an MI355X.

Routes.  ceg_pairs_energy with the default switches (k_pairs_frac where the handle is fast), with CEG_HIP_PAIRS_FRAC=0 (k_pairs, fast
wrap) and with CEG_HIP_PAIRS_WRAP=0 (k_pairs, the reference's distance); column 2 of ceg_mc_trial from k_mc_trial
(CEG_HIP_MC_WAVE_MIN huge), from the wave kernels (= 0; k_mcw_pairs_frac where the handle is fast) and from k_mcw_pairs
(CEG_HIP_MC_FRAC=0 as well); ceg_mc_trial_insert with the default switches.

Criterion.  _assert_energies of test_gpu_consumers.py at its rtol = 1e-9, per table ENTRY -- and, within an entry, per domain of the
arithmetic (r^2 < 0.25: libm-grade; 0.25 <= r^2 < 1: polynomials; r^2 >= 1: polynomials or records) on that domain's own scale,
since the scale of a whole entry is set by its pairs at 0.05-0.2 A, ten and more decades above the values beyond 1 A.  HardSphere
decisions are the oracle's everywhere on the literal route and for |delta| >= 1e-9 on the routes with the approximate distance; inside that
band those routes may answer either way ("Pair rules").  Every figure is printed (`PAIRRULE` lines:
profiles/pair_rule_arithmetic.txt is a copy) before anything is asserted."""
import numpy as np
import pytest

from ceg_hip import _abi

import pair_rule_cases as PC
from test_gpu_consumers import _RawMc, _assert_energies, _pairs_gpu

pytestmark = pytest.mark.gpu

SWITCHES = ("CEG_HIP_PAIRS_FRAC", "CEG_HIP_PAIRS_WRAP", "CEG_HIP_MC_WAVE_MIN", "CEG_HIP_MC_FRAC", "CEG_HIP_MC_SPLIT_MAX", "CEG_HIP_MC_CELLS",
            "CEG_HIP_MC_BIN", "CEG_HIP_PAIRS_PER_WAVE")
ROUTES = {          # name -> (entry point, environment)
    "pairs": ("pairs", {}),
    "pairs/FRAC=0": ("pairs", {"CEG_HIP_PAIRS_FRAC": "0"}),
    "pairs/WRAP=0": ("pairs", {"CEG_HIP_PAIRS_WRAP": "0"}),
    "mc/workgroup": ("trial", {"CEG_HIP_MC_WAVE_MIN": "1000000000"}),
    "mc/wave": ("trial", {"CEG_HIP_MC_WAVE_MIN": "0"}),
    "mc/wave/FRAC=0": ("trial", {"CEG_HIP_MC_WAVE_MIN": "0", "CEG_HIP_MC_FRAC": "0"}),
    "mc/insert": ("insert", {}),
}
LITERAL = ("pairs/WRAP=0",)           # routes that measure the reference's distance for every pair
BANDS = (("r2<0.25", 0.0, 0.25), ("0.25<=r2<1", 0.25, 1.0), ("r2>=1", 1.0, np.inf))
_RESULTS = {}


def _switch(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _deviation(got, ref):
    """the measure of _assert_energies, without the assertions: worst |got - ref| / max(|ref|, 1e-3 upper quartile of |ref|)"""
    fin = np.isfinite(ref) & np.isfinite(got)
    if not fin.any():
        return 0.0
    allfin = np.isfinite(ref)
    scale = float(np.percentile(np.abs(ref[allfin]), 75))
    den = np.maximum(np.abs(ref[fin]), 1e-3 * scale)
    err = np.abs(got[fin] - ref[fin])
    return float(np.max(np.where(err == 0.0, 0.0, err / np.where(den > 0.0, den, 1e-300))))


def _single(lib, oracle, monkeypatch, name, which):
    """{'cases', 'ref': [per case], 'r2': [per case], 'got': {route: [per case]}} of a table in a cell, run once"""
    key = (name, which)
    if key in _RESULTS:
        return _RESULTS[key]
    t, mat = PC.table(name), PC.cell(which)
    inv = np.linalg.inv(mat)
    cases = PC.single_pairs(t, mat)
    ref = [oracle.single_contribution_vdw_raw(mat, inv, *t.args(), c.atom[None], [c.kind], [0], c.trial, [0], -1) for c in cases]
    r2 = [PC.literal_r2(mat, inv, c.atom, c.trial) for c in cases]
    got = {route: [] for route in ROUTES}
    _switch(monkeypatch, {})
    mc = _RawMc(lib, mat, *t.args())
    try:
        for c in cases:
            mc.set_guests(np.stack([c.atom, c.parked]), [c.kind, 0], [0, 1, 2])
            for route, (entry, env) in ROUTES.items():
                _switch(monkeypatch, env)
                if entry == "pairs":
                    out = _pairs_gpu(lib, mat, *t.args(), c.atom[None], [c.kind], [0], c.trial, [0], -1)
                elif entry == "trial":
                    out = mc.trial(1, c.trial)[1:].copy()
                else:
                    out = mc.trial_insert([0], c.trial).copy()
                got[route].append(out)
    finally:
        _switch(monkeypatch, {})
        mc.close()
    _RESULTS[key] = {"t": t, "cases": cases, "ref": ref, "r2": r2, "got": got}
    return _RESULTS[key]


def _by_entry(res, e, what):
    idx = [i for i, c in enumerate(res["cases"]) if c.entry == e]
    return np.concatenate([what[i] for i in idx])


def _undecided(res, e):
    """placements within |delta| < 1e-9 of a sphere radius: the routes with the approximate distance may take them either way"""
    tag = _by_entry(res, e, [c.tag for c in res["cases"]])
    delta = _by_entry(res, e, [c.delta for c in res["cases"]])
    return (tag == PC.TAG_SPHERE) & (np.abs(delta) < 1e-9)


CASES = [(name, "triangular") for name in PC.TABLES] + [(name, "rotated") for name in PC.ROTATED]


@pytest.mark.parametrize("name,which", CASES, ids=[f"{n}-{w}" for n, w in CASES])
def test_single_pairs(hip_lib, oracle, monkeypatch, name, which):
    """every entry of the table, one pair per output, on every route: NaN / Inf patterns and HardSphere decisions, values per entry and
    per arithmetic domain at 1e-9, routes among each other at 1e-10"""
    res = _single(hip_lib, oracle, monkeypatch, name, which)
    t = res["t"]
    failures = []
    rows = []
    for e in range(len(t.entries)):
        ename = t.entry_name(e)
        ref = _by_entry(res, e, res["ref"])
        r2 = _by_entry(res, e, res["r2"])
        loose = _undecided(res, e)
        base = _by_entry(res, e, res["got"]["pairs"])
        for route in ROUTES:
            got = _by_entry(res, e, res["got"][route])
            what = f"{name}/{which}/{route}/{ename}"
            if np.isnan(got).any() or np.isnan(ref).any():
                failures.append(f"{what}: NaN")
                continue
            # HardSphere decisions
            decided = np.ones(len(ref), dtype=bool) if route in LITERAL else ~loose
            wrong = decided & (np.isinf(got) != np.isinf(ref))
            if wrong.any():
                failures.append(f"{what}: {int(wrong.sum())} HardSphere decisions differ from the oracle's")
            if not np.all(got[np.isinf(got)] == np.inf):
                failures.append(f"{what}: -Inf")
            keep = decided | (np.isinf(got) == np.isinf(ref))          # inside the band: 0 or Inf, compared when it is the oracle's answer
            keep &= ~wrong
            devs = []
            for label, sel in [("entry", np.ones(len(ref), dtype=bool))] + [(b, (r2 >= lo) & (r2 < hi)) for b, lo, hi in BANDS]:
                sel = sel & keep
                if not (sel & np.isfinite(ref)).any():
                    devs.append(float("nan"))
                    continue
                devs.append(_deviation(got[sel], ref[sel]))
                try:
                    with np.errstate(invalid="ignore"):          # (an entry of zeros -- `empty` -- has scale 0: 0 <= 0 holds, the message divides)
                        _assert_energies(got[sel], ref[sel], f"{what}, {label}")
                except AssertionError as err:
                    failures.append(str(err).splitlines()[0])
            # the routes among each other (the form of test_pairs_fractional_kernel), against the default ceg_pairs_energy route
            fin = np.isfinite(ref) & np.isfinite(got) & np.isfinite(base)
            agree = 0.0
            if fin.any() and route != "pairs":
                floor = 1e-3 * np.percentile(np.abs(ref[np.isfinite(ref)]), 75)
                agree = float(np.max(np.abs(got[fin] - base[fin]) / (np.abs(base[fin]) + floor + 1e-300)))
                if agree > 1e-10:
                    failures.append(f"{what}: differs from the default route by {agree:.3e} (1e-10)")
            rows.append(f"PAIRRULE {name:13s} {which:10s} {route:15s} {ename:22s} " + " ".join(f"{d:9.2e}" for d in devs) + f" {agree:9.2e}")
    print(f"PAIRRULE table         cell       route           entry                      entry   r2<0.25 0.25..1     r2>=1  vs pairs")
    print("\n".join(rows))
    assert not failures, "\n".join(failures)


def test_frac_switch_selects_another_kernel(hip_lib, oracle, monkeypatch):
    """for the `fast` table the default route (k_pairs_frac: records) and CEG_HIP_PAIRS_FRAC=0 (k_pairs: polynomials) differ in at least
    one finite value -- within the 1e-10 asserted above --, and so do the two wave routes of ceg_mc_trial"""
    res = _single(hip_lib, oracle, monkeypatch, "fast", "triangular")
    for a, b in (("pairs", "pairs/FRAC=0"), ("mc/wave", "mc/wave/FRAC=0")):
        x, y = np.concatenate(res["got"][a]), np.concatenate(res["got"][b])
        fin = np.isfinite(x) & np.isfinite(y)
        assert (x[fin] != y[fin]).any(), (a, b)


def test_order_of_the_table(hip_lib, oracle, monkeypatch):
    """alpha0_first and alpha0_last hold the same entries under other kind numbers: the same physical pairs get the same energies
    (1e-10, the form of the route comparison) on every route"""
    first = _single(hip_lib, oracle, monkeypatch, "alpha0_first", "triangular")
    last = _single(hip_lib, oracle, monkeypatch, "alpha0_last", "triangular")
    ta, tb = first["t"], last["t"]
    failures = []
    for e in range(len(ta.entries)):
        assert ta.entry_name(e) == tb.entry_name(e)
        ref = _by_entry(first, e, first["ref"])
        assert np.array_equal(ref, _by_entry(last, e, last["ref"]), equal_nan=True)          # the same pairs, by the oracle
        loose = _undecided(first, e)
        fin_ref = np.isfinite(ref)
        floor = 1e-3 * np.percentile(np.abs(ref[fin_ref]), 75) if fin_ref.any() else 0.0
        for route in ROUTES:
            x, y = _by_entry(first, e, first["got"][route]), _by_entry(last, e, last["got"][route])
            fin = np.isfinite(x) & np.isfinite(y)
            if not np.array_equal(np.isfinite(x)[~loose], np.isfinite(y)[~loose]):
                failures.append(f"{route}/{ta.entry_name(e)}: Inf patterns differ")
            d = float(np.max(np.abs(x[fin] - y[fin]) / (np.abs(y[fin]) + floor + 1e-300))) if fin.any() else 0.0
            print(f"PAIRRULE order {route:15s} {ta.entry_name(e):22s} {d:9.2e}")
            if d > 1e-10:
                failures.append(f"{route}/{ta.entry_name(e)}: alpha0_first and alpha0_last differ by {d:.3e}")
    assert not failures, "\n".join(failures)


CROWDS = [(name, "triangular") for name in PC.TABLES] + [(name, "rotated") for name in PC.ROTATED]


@pytest.mark.parametrize("name,which", CROWDS, ids=[f"{n}-{w}" for n, w in CROWDS])
def test_crowd(hip_lib, oracle, monkeypatch, name, which):
    """600 guest atoms of every kind in a 14 A ball, molecules of 1, 3, 4 and 6 atoms: every placement queues several batches of pairs
    (records, walked entries, pairs below 1 A and below 0.5 A in one batch), sums against the oracle at 1e-9 on every route"""
    t, mat = PC.table(name), PC.cell(which)
    inv = np.linalg.inv(mat)
    cr = PC.crowd(t, mat)
    failures, rows = [], []
    _switch(monkeypatch, {})
    mc = _RawMc(hip_lib, mat, *t.args())
    try:
        for m in PC.CROWD_SIZES:
            trial, tk = cr.trials[m], [0] * m
            ref = oracle.single_contribution_vdw_raw(mat, inv, *t.args(), cr.pos, cr.kinds, cr.mol, trial, tk, -1)
            first = np.arange(len(cr.pos) + 1, dtype=np.int32)
            for route, (entry, env) in ROUTES.items():
                _switch(monkeypatch, {})
                if entry == "trial":
                    mc.set_guests(np.concatenate([cr.pos, cr.parked[m]]), np.concatenate([cr.kinds, tk]), np.concatenate([first, [len(cr.pos) + m]]))
                elif entry == "insert":
                    mc.set_guests(cr.pos, cr.kinds, first)
                _switch(monkeypatch, env)
                if entry == "pairs":
                    got = _pairs_gpu(hip_lib, mat, *t.args(), cr.pos, cr.kinds, cr.mol, trial, tk, -1)
                elif entry == "trial":
                    got = mc.trial(len(cr.pos), trial)[1:].copy()
                else:
                    got = mc.trial_insert(tk, trial).copy()
                rows.append(f"PAIRRULE crowd {name:13s} {which:10s} {route:15s} {m} atoms {_deviation(got, ref):9.2e}")
                try:
                    _assert_energies(got, ref, f"crowd {name}/{which}/{route}, {m} atoms")
                except AssertionError as err:
                    failures.append(str(err).splitlines()[0])
    finally:
        _switch(monkeypatch, {})
        mc.close()
    print("\n".join(rows))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", ["fast", "edge_slow"])
def test_baseline_inter_of_the_crowd(hip_lib, oracle, monkeypatch, name):
    """the guest-guest term of ceg_mc_baseline on the crowd itself: half the sum of every molecule's single_contribution_vdw, within
    1e-9 of the sum of their absolute values + 1e-7 per molecule (the tolerance of test_gpu_mc_baseline.py)"""
    t, mat = PC.table(name), PC.cell("triangular")
    cr = PC.crowd(t, mat)
    per_mol = PC.crowd_pair_sums(oracle, t, mat, cr)
    assert np.isfinite(per_mol).all()
    want, tol = 0.5 * float(per_mol.sum()), 1e-9 * float(np.abs(per_mol).sum()) + 1e-7 * len(per_mol)
    _switch(monkeypatch, {})
    mc = _RawMc(hip_lib, mat, *t.args())
    try:
        mc.set_guests(cr.pos, cr.kinds, np.arange(len(cr.pos) + 1, dtype=np.int32))
        for flags in (0, _abi.MC_BASELINE_REFRESH):
            rec = np.zeros(1, dtype=_abi.MC_BASELINE_DTYPE)
            _abi.check(hip_lib, hip_lib.ceg_mc_baseline(mc.h, flags, rec.ctypes.data))
            got = float(rec[0]["inter"])
            print(f"PAIRRULE baseline {name:13s} flags {flags}: device {got!r}, oracle {want!r}, |difference| {abs(got - want):.3e}, tolerance {tol:.3e}")
            assert (int(rec[0]["nmol"]), int(rec[0]["natoms"])) == (len(cr.pos), len(cr.pos))
            assert abs(got - want) <= tol
            assert float(rec[0]["framework_vdw"]) == 0.0 and float(rec[0]["recip_guests"]) == 0.0
    finally:
        mc.close()
