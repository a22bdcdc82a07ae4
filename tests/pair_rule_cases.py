"""Cases for the guest-guest pair arithmetic (energy.jl:397-427) over every rule kind and every switch of
the arithmetic: pair tables, single-pair placements on the switch points, a crowd that fills the hit queues.  No tests in here:
``tests/test_pair_rule_cases_host.py`` checks this module on the CPU, ``tests/test_gpu_pair_rules.py`` runs it on the GPU.

Tables.  A table is a list of ENTRIES (rule sums); guest kind g meets trial kind 0 through entry ``entry_of_kind[g]``, the table
is symmetric and every other pair of kinds has no rule at all -- except in ``wide``, whose other pairs are filled as well, since
a 36-kind table with 71 short entries would stay far below the budgets it is there to exceed.  The CoulombEwaldDirect entry with
alpha = 0 is part of the two ``alpha0_*`` tables only: a table that holds it has two different alpha (0 and 0.265) and therefore
no erfc(alpha r)/r records, whatever the order of its kinds.

``predicted`` restates the conditions the create functions decide by (documented in DESIGN.md and the headers) without calling
the library: fast <=> alpha cutoff <= 5 (1 - 1e-9) for every CoulombEwaldDirect rule and B cutoff <= 700 for every Buckingham /
Exponential rule; erfc records <=> fast, one alpha > 0 shared by all CoulombEwaldDirect rules, cutoff^2 > 1; the table is staged
in LDS when 40 B per rule + 4 B per offset fit in 48 KB (ceg_pairs) / 32 KB (ceg_mc)."""
import math
import zlib

import numpy as np

from ceg_hip import _abi
from ceg_hip.hostmirror.constants import COULOMBIC_CONVERSION_FACTOR as COULOMBIC
from ceg_hip.hostmirror.interactions import FF

LD = np.longdouble
CUTOFF = 12.0
ALPHA = 0.265
SPHERE = 1.5                      # summed radius of the HardSphere + Buckingham + CED entry
SPHERE_ALONE = 0.85 + 0.6         # the HardSphere-only entry
TABLES = ("fast", "edge_fast", "edge_slow", "alpha0_first", "alpha0_last", "two_alphas", "steep", "wide", "short")
ROTATED = ("fast", "alpha0_first", "wide")            # tables that also run in the rotated (general-matrix) cell
GUEST_FRAC = ((0.31, 0.52, 0.47), (0.02, 0.97, 0.5), (1.99, -0.98, 0.01))     # interior, near a face, outside the unit cell
ALPHA0 = "CED(alpha=0)"


# ------------------------------------------------------------------ rules and entries
def _lj(eps, sigma, cutoff):
    x6 = (sigma / cutoff) ** 6
    return (int(FF.LennardJones), (eps, sigma, 0.0), 4 * eps * x6 * (x6 - 1))


def _buck(a, b, c, cutoff):
    return (int(FF.Buckingham), (a, b, c), a * math.exp(-b * cutoff) - c / cutoff ** 6)


def _ced(alpha, q1, q2, shift=0.0):
    return (int(FF.CoulombEwaldDirect), (alpha, q1, q2), shift)


def entries(cutoff=CUTOFF, alpha=(ALPHA, ALPHA), exp_b=3.3):
    """[(name, [(kind, p, shift), ...])] -- ``alpha``: the two values the CoulombEwaldDirect rules take in turn"""
    a = [alpha[i % 2] for i in range(5)]
    return [
        ("LJ", [_lj(120.0, 3.2, cutoff)]),
        ("LJ+CED", [_lj(85.0, 3.05, cutoff), _ced(a[0], 0.7, -0.9)]),
        ("CED", [_ced(a[1], 0.8, 0.6, 0.37)]),
        ("HS+Buckingham+CED", [_buck(5.0e6, 3.6, 4.0e4, cutoff), (int(FF.HardSphere), (SPHERE, 0.0, 0.0), 0.0), _ced(a[2], 1.0, -0.8)]),
        ("HS", [(int(FF.HardSphere), (0.85, 0.6, 0.0), 0.25)]),
        ("Buckingham", [_buck(8.0e5, 3.1, 2.5e3, cutoff)]),
        ("Monomial", [(int(FF.Monomial), (3.0e5, 9.0, 0.0), 3.0e5 / cutoff ** 9)]),
        ("Exponential", [(int(FF.Exponential), (4.0e6, exp_b, 0.0), 4.0e6 * math.exp(-exp_b * cutoff))]),
        ("Coulomb", [(int(FF.Coulomb), (0.6, -0.7, 0.0), COULOMBIC * 0.6 * -0.7 / cutoff)]),
        ("NoInteraction", [(int(FF.NoInteraction), (0.0, 0.0, 0.0), 1.75)]),
        ("empty", []),
        ("LJ+LJ", [_lj(60.0, 2.9, cutoff), _lj(30.0, 3.6, cutoff)]),
        ("LJ+NoInteraction+CED", [_lj(100.0, 3.3, cutoff), (int(FF.NoInteraction), (0.0, 0.0, 0.0), -0.5), _ced(a[3], -0.6, -0.5, 0.11)]),
    ]


ALPHA0_ENTRY = (ALPHA0, [_ced(0.0, -0.5, 0.9, -2.5)])


class Table:
    def __init__(self, name, cutoff, ents, entry_of_kind, filled=False):
        self.name, self.cutoff, self.entries = name, float(cutoff), ents
        self.entry_of_kind = list(entry_of_kind)
        self.nkinds = nk = len(self.entry_of_kind)
        rules, offsets = [], [0]
        for a in range(nk):
            for b in range(nk):
                if a == 0 or b == 0:
                    e = self.entry_of_kind[a + b]
                elif filled:
                    e = (a + b) % len(ents)
                else:
                    e = None
                if e is not None:
                    rules += ents[e][1]
                offsets.append(len(rules))
        self.rules = np.zeros(max(len(rules), 1), dtype=_abi.RULE_DTYPE)
        for q, (kind, p, shift) in enumerate(rules):
            self.rules[q]["kind"] = kind
            self.rules[q]["p"] = p
            self.rules[q]["shift"] = shift
        self.nrules = len(rules)
        self.offsets = np.asarray(offsets, dtype=np.int32)

    def entry_rules(self, e):
        return self.entries[e][1]

    def entry_name(self, e):
        return self.entries[e][0]

    def kinds_of_entry(self, e):
        return [g for g, x in enumerate(self.entry_of_kind) if x == e]

    def spheres(self, e):
        """the summed radii of the HardSphere rules of entry e"""
        return [p[0] + p[1] for kind, p, _s in self.entry_rules(e) if kind == int(FF.HardSphere)]

    def hard_kinds(self):
        return [g for g, e in enumerate(self.entry_of_kind) if self.spheres(e)]

    def args(self):
        """the leading arguments of _pairs_gpu / _RawMc / oracle.single_contribution_vdw_raw after the matrices"""
        return (self.cutoff ** 2, self.rules, self.offsets, self.nkinds, COULOMBIC)


_TABLES = {}


def table(name):
    if name in _TABLES:
        return _TABLES[name]
    n = len(entries())
    plain = list(range(n))
    if name == "fast":
        t = Table(name, CUTOFF, entries(), plain)
    elif name == "edge_fast":
        t = Table(name, CUTOFF, entries(alpha=(4.99 / CUTOFF,) * 2), plain)
    elif name == "edge_slow":
        t = Table(name, CUTOFF, entries(alpha=(5.01 / CUTOFF,) * 2), plain)
    elif name == "alpha0_first":
        t = Table(name, CUTOFF, entries() + [ALPHA0_ENTRY], [n] + plain)
    elif name == "alpha0_last":
        t = Table(name, CUTOFF, entries() + [ALPHA0_ENTRY], plain + [n])
    elif name == "two_alphas":
        t = Table(name, CUTOFF, entries(alpha=(0.2, 0.3)), plain)
    elif name == "steep":
        t = Table(name, CUTOFF, entries(exp_b=701.0 / CUTOFF), plain)
    elif name == "wide":
        t = Table(name, CUTOFF, entries(), [g % n for g in range(36)], filled=True)
    elif name == "short":
        t = Table(name, 0.9, entries(cutoff=0.9), plain)
    else:
        raise KeyError(name)
    _TABLES[name] = t
    return t


def rejected_table():
    """one UndefinedInteraction rule: both create functions answer CEG_ERR_RULE before anything touches a device"""
    t = Table("rejected", CUTOFF, [("Undefined", [(int(FF.UndefinedInteraction), (0.0, 0.0, 0.0), 0.0)])], [0])
    return t


def predicted(t):
    """{'fast', 'erfc', 'pairs_lds', 'mc_lds'} from the documented conditions alone (see the module docstring)"""
    fast = True
    alphas = set()
    for r in t.rules[:t.nrules]:
        kind, p = int(r["kind"]), r["p"]
        if kind == int(FF.CoulombEwaldDirect):
            alphas.add(float(p[0]))
            if not (p[0] >= 0.0 and p[0] * t.cutoff <= 5.0 * (1.0 - 1e-9)):
                fast = False
        if kind in (int(FF.Buckingham), int(FF.Exponential)) and not (p[1] >= 0.0 and p[1] * t.cutoff <= 700.0):
            fast = False
    erfc = fast and len(alphas) == 1 and min(alphas) > 0.0 and t.cutoff ** 2 > 1.0
    nbytes = 40 * max(t.nrules, 1) + 4 * (t.nkinds * t.nkinds + 1)
    return {"fast": fast, "erfc": erfc, "pairs_lds": nbytes <= 48 * 1024, "mc_lds": nbytes <= 32 * 1024, "bytes": nbytes}


INTENDED = {          # (fast, erfc records, table in LDS of ceg_pairs, of ceg_mc)
    "fast": (True, True, True, True), "edge_fast": (True, True, True, True), "edge_slow": (False, False, True, True),
    "alpha0_first": (True, False, True, True), "alpha0_last": (True, False, True, True), "two_alphas": (True, False, True, True),
    "steep": (False, False, True, True), "wide": (True, True, False, False), "short": (True, False, True, True),
}


# ------------------------------------------------------------------ cells
def cell(which):
    """the 40 A skewed upper-triangular cell of test_pairs_cutoff_decision_is_the_references, or a rotated copy (general matrix)"""
    mat = np.array([[40.0, 0, 0], [3.0, 40.0, 0], [-2.0, 4.0, 40.0]]).T
    if which == "rotated":
        q = np.array([0.83, -0.31, 0.42, 0.19])
        a, b, c, d = q / np.linalg.norm(q)
        rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                        [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                        [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
        mat = rot @ mat
    else:
        assert which == "triangular"
    return mat


def literal_r2(mat, inv, atom, trial):
    """unsafe_periodic_distance2! (utils.jl:294-302) in numpy with the reference's operation order: the r^2 the rules are given"""
    d = np.asarray(trial, dtype=np.float64).reshape(-1, 3) - np.asarray(atom, dtype=np.float64).reshape(-1, 3)

    def mv(m, v):
        return [(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)]
    f = mv(inv, (d[:, 0], d[:, 1], d[:, 2]))
    w = []
    for x in f:
        s = x + 0.5
        w.append((s - np.floor(s)) - 0.5)
    v = mv(mat, w)
    r2 = np.zeros(len(d))
    for x in v:
        r2 = r2 + x * x
    return r2


# ------------------------------------------------------------------ single pairs
TAG_LOG, TAG_QUARTER, TAG_ONE, TAG_EDGE, TAG_SPHERE = range(5)
THRESHOLD_DELTAS = (0.0, 2e-16, -2e-16, 1e-12, -1e-12, 1e-9, -1e-9)
SPHERE_DELTAS = (1e-6, -1e-6, 1e-8, -1e-8, 1e-9, -1e-9, 0.0, 3e-16, -3e-16, 1e-14, -1e-14)
NDIR = 2              # directions per switch-point distance and guest position


def table_edges(cutoff=CUTOFF):
    """lower ends of the erfc-record intervals, 2^k (1 + j/32), inside (1, cutoff^2): a spread over every octave, with the upper end of
    the first interval and the lower ends of the last two intervals a pair inside the cutoff can reach"""
    c2 = cutoff * cutoff
    out = []
    for k in range(0, 8):
        for j in (0, 1, 5, 11, 16, 23, 31):
            s = 2.0 ** k * (1.0 + j / 32.0)
            if 1.0 < s < c2 * (1.0 - 4e-9):
                out.append(s)
    top = math.floor(math.log2(c2))
    j_last = int((c2 / 2.0 ** top - 1.0) * 32.0 - 1e-9)
    for j in (j_last, j_last - 1):
        if j >= 0:
            s = 2.0 ** top * (1.0 + j / 32.0)
            if s not in out and 1.0 < s < c2 * (1.0 - 4e-9):
                out.append(s)
    return sorted(out)


def switch_points(t, e):
    """(target r^2, delta, tag) of the switch-point distances of entry e: r^2 = target (1 + delta)"""
    pts = []
    for d in THRESHOLD_DELTAS:
        pts.append((0.25, d, TAG_QUARTER))
        pts.append((1.0, d, TAG_ONE))
    for s in table_edges():
        pts.append((s, 1e-9, TAG_EDGE))
        pts.append((s, -1e-9, TAG_EDGE))
    for s in t.spheres(e):
        for d in SPHERE_DELTAS:
            pts.append((s * s, d, TAG_SPHERE))
    return pts


class PairCase:
    """one guest atom of kind ``kind`` (entry ``entry``) at ``atom``; trial[i] is one atom of kind 0 at distance sqrt(target[i] (1 + delta[i]))"""
    def __init__(self, entry, kind, ipos, atom, trial, target, delta, tag):
        self.entry, self.kind, self.ipos, self.atom, self.trial = entry, kind, ipos, atom, trial
        self.parked = None            # set by single_pairs: where the molecule on trial of ceg_mc_trial sits, out of everybody's reach
        self.target, self.delta, self.tag = target, delta, tag


def single_pairs(t, mat, nlog=300):
    """the PairCases of a table in a cell: every entry x the three guest positions (for ``wide`` each entry through one of its kinds,
    in turn)"""
    cases = []
    for e in range(len(t.entries)):
        kinds = t.kinds_of_entry(e)
        pts = switch_points(t, e)
        for ipos, frac in enumerate(GUEST_FRAC):
            rng = np.random.default_rng(zlib.crc32(f"{t.entry_name(e)}/{ipos}".encode()))        # (the same placements in every table)
            atom = mat @ np.array(frac)
            r_log = np.exp(np.linspace(math.log(0.05), math.log(0.999 * t.cutoff), nlog)) * (1.0 + rng.uniform(-1e-3, 1e-3, nlog))
            r_log = np.minimum(r_log, 0.999 * t.cutoff)
            target = np.concatenate([r_log ** 2] + [np.repeat(s, NDIR) for s, _d, _g in pts])
            delta = np.concatenate([np.zeros(nlog)] + [np.repeat(d, NDIR) for _s, d, _g in pts])
            tag = np.concatenate([np.full(nlog, TAG_LOG)] + [np.repeat(g, NDIR) for _s, _d, g in pts]).astype(np.int32)
            n = len(target)
            u = rng.normal(size=(n, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            r = np.sqrt(target * (1.0 + delta))
            trial = atom[None] + r[:, None] * u
            third = np.arange(n) % 3 == (ipos % 3)
            trial[third] += (mat @ rng.integers(-2, 3, (3, int(third.sum())))).T          # other images of the same placement
            cases.append(PairCase(e, kinds[ipos % len(kinds)], ipos, atom, trial[:, None, :], target, delta, tag))
            cases[-1].parked = atom + mat @ np.array([0.5, 0.5, 0.5])
    return cases


# ------------------------------------------------------------------ the checker, restated in longdouble
def rule_terms_ld(rule, r2):
    """(value, shift, size) of one rule at r2 (float64 array) in longdouble -- interactions.jl:367-406 as the oracle restates them; the
    two erfc kinds take math.erfc of the float64 argument alpha * sqrt(r2) the oracle itself forms.  size: the sum of the absolute
    values of the terms the formula subtracts from one another (4 eps x^12 and 4 eps x^6; A exp(-B r) and C / r^6), |value| otherwise:
    what a rounding error of the evaluation is proportional to"""
    size = None
    kind, p, shift = rule
    r2l = np.asarray(r2, dtype=LD)
    p0, p1, p2 = (LD(float(x)) for x in p)
    if kind == int(FF.LennardJones):
        q = (p1 * p1) / r2l
        x6 = q * q * q
        v = LD(4) * p0 * x6 * (x6 - LD(1))
        size = np.abs(LD(4) * p0) * (x6 * x6 + x6)
    elif kind == int(FF.HardSphere):
        s = float(p[0]) + float(p[1])
        v = np.where(np.asarray(r2) < s * s, LD(np.inf), LD(0))
    elif kind == int(FF.NoInteraction):
        v = np.zeros(len(r2l), dtype=LD)
    elif kind == int(FF.Monomial):
        v = p0 / np.power(r2l, p1 / LD(2))
    elif kind == int(FF.CoulombEwaldDirect):
        rd = np.sqrt(np.asarray(r2, dtype=np.float64))
        ef = np.array([math.erfc(float(p[0]) * float(x)) for x in rd], dtype=LD)
        v = LD(COULOMBIC) * p1 * p2 * ef / np.sqrt(r2l)
    elif kind == int(FF.Coulomb):
        v = LD(COULOMBIC) * p0 * p1 / np.sqrt(r2l)
    elif kind == int(FF.Buckingham):
        r = np.sqrt(r2l)
        v = p0 * np.exp(-p1 * r) - p2 / (r2l * r2l * r2l)
        size = np.abs(p0 * np.exp(-p1 * r)) + np.abs(p2 / (r2l * r2l * r2l))
    elif kind == int(FF.Exponential):
        v = p0 * np.exp(-p1 * np.sqrt(r2l))
    else:
        raise ValueError(kind)
    if size is None:
        size = np.where(np.isfinite(v), np.abs(v), LD(0))
    return v, LD(float(shift)), size


def entry_energy_ld(t, e, r2):
    """(rule sum of entry e at r2 where r2 < cutoff^2 -- 0 outside --, sum of the absolute values of its terms and shifts)"""
    r2 = np.asarray(r2, dtype=np.float64)
    total = np.zeros(len(r2), dtype=LD)
    size = np.zeros(len(r2), dtype=LD)
    for rule in t.entry_rules(e):
        v, s, sz = rule_terms_ld(rule, r2)
        total = total + (v - s)
        size = size + sz + abs(s)
    inside = r2 < t.cutoff ** 2
    return np.where(inside, total, LD(0)), np.where(inside, size, LD(0))


def exp_argument_size(t, e, r2):
    """sum over the Buckingham / Exponential rules of entry e of B r |A exp(-B r)|: times 2^-52 what the two float64 roundings of the
    argument B sqrt(r2) (square root, product) move the term by -- negligible (< 1e-14 of the term) up to B r = 45, 1.6e-13 at 701"""
    r = np.sqrt(np.asarray(r2, dtype=LD))
    out = np.zeros(len(r), dtype=LD)
    for kind, p, _s in t.entry_rules(e):
        if kind in (int(FF.Buckingham), int(FF.Exponential)):
            out = out + LD(float(p[1])) * r * np.abs(LD(float(p[0])) * np.exp(-LD(float(p[1])) * r))
    return out


# ------------------------------------------------------------------ the crowd
CROWD_SIZES = (1, 3, 4, 6)
CROWD_CENTRE_FRAC = (0.08, 0.5, 0.93)          # the ball crosses two faces of the cell


class Crowd:
    def __init__(self, pos, kinds, trials, parked):
        self.pos, self.kinds, self.trials, self.parked = pos, kinds, trials, parked
        self.mol = np.arange(len(pos), dtype=np.int32)


def crowd(t, mat, natoms=600, radius=14.0, sep=1.2, nplace=64):
    """``natoms`` guest atoms of mixed kinds (a quarter of kind 0) in a ball, at least ``sep`` apart; no HardSphere kind within 1.6 A of a
    kind-0 atom, so that the pair sum of the state itself (ceg_mc_baseline) is finite.  trials[m]: ``nplace`` placements of a rigid
    molecule of m atoms of kind 0, three in eight with their first atom 0.3-1 A from a guest atom, a third shifted by lattice vectors.
    parked[m]: where such a molecule sits while it is the molecule on trial of ceg_mc_trial (its own atoms are excluded)."""
    rng = np.random.default_rng(zlib.crc32(f"crowd/{t.name}".encode()))
    centre = mat @ np.array(CROWD_CENTRE_FRAC)
    pts = []
    while len(pts) < natoms:
        c = rng.uniform(-radius, radius, 3)
        if c @ c > radius * radius:
            continue
        if pts and np.min(np.sum((np.asarray(pts) - c) ** 2, axis=1)) < sep * sep:
            continue
        pts.append(c)
    rel = np.asarray(pts)
    kinds = rng.integers(0, t.nkinds, natoms).astype(np.int32)
    kinds[rng.uniform(size=natoms) < 0.25] = 0
    hard = set(t.hard_kinds())
    soft = [g for g in range(1, t.nkinds) if g not in hard]
    zero = rel[kinds == 0]
    for i in range(natoms):
        if int(kinds[i]) in hard and np.min(np.sum((zero - rel[i]) ** 2, axis=1)) < 1.6 ** 2:
            kinds[i] = soft[i % len(soft)]
    pos = rel + centre
    inner = np.nonzero(np.sum(rel * rel, axis=1) < 10.0 ** 2)[0]      # (a trial atom at the rim of the ball would see too few guests)
    trials, parked = {}, {}
    for m in CROWD_SIZES:
        shape = np.zeros((m, 3))
        for a in range(1, m):
            step = rng.normal(size=3)
            shape[a] = shape[a - 1] + 1.2 * step / np.linalg.norm(step)
        out = np.empty((nplace, m, 3))
        for i in range(nplace):
            q = rng.normal(size=4)
            a, b, c, d = q / np.linalg.norm(q)
            rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                            [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                            [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
            if i % 8 < 3:
                j = int(rng.choice(inner))
                u = rng.normal(size=3)
                first = pos[j] + rng.uniform(0.3, 1.0) * u / np.linalg.norm(u)
            else:
                while True:
                    first = rng.uniform(-6.0, 6.0, 3)
                    if first @ first <= 36.0:
                        break
                first = first + centre
            out[i] = first + shape @ rot.T
            if i % 3 == 1:
                out[i] += mat @ rng.integers(-2, 3, 3)
        trials[m] = out
        parked[m] = mat @ np.array([0.55, 0.1, 0.4]) + shape
    return Crowd(pos, kinds, trials, parked)


def crowd_pair_sums(oracle, t, mat, cr):
    """single_contribution_vdw of every (one-atom) molecule of the crowd where it is: the inter term of baseline_energy is half their sum"""
    inv = np.linalg.inv(mat)
    return np.array([oracle.single_contribution_vdw_raw(mat, inv, *t.args(), cr.pos, cr.kinds, cr.mol, cr.pos[i][None, None, :],
                                                        [int(cr.kinds[i])], i)[0] for i in range(len(cr.pos))])
