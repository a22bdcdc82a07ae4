"""Plan-time detection of the uniform class of the grid kernels (no GPU): ``ceg_uniform_class`` runs the classification of
``ceg_plan_create`` -- rule conversion, per-kind fast records, ``detect_uniform_class`` -- on hand-made atom and rule tables.
0: per-candidate Lennard-Jones records; 1 (uni_lj): one bit-identical Lennard-Jones record for every kind that is present and has
a rule; 2 (uni_q): 1, and one bit-identical charge on every atom of those kinds."""
import numpy as np
import pytest

from ceg_hip import _abi

LJ, BUCK, NONE = 3, 4, 8          # ceg_kind of include/ceg_hip.h
CUTOFF2 = 144.0


def _table(per_kind):
    """per_kind: list (one entry per kind) of lists of (kind, p0, p1, p2, shift) -> (rules, offsets)"""
    flat = [r for run in per_kind for r in run]
    rules = np.zeros(max(len(flat), 1), dtype=_abi.RULE_DTYPE)
    for t, (k, p0, p1, p2, sh) in enumerate(flat):
        rules[t]["kind"] = k
        rules[t]["p"] = (p0, p1, p2)
        rules[t]["shift"] = sh
    offsets = np.cumsum([0] + [len(run) for run in per_kind]).astype(np.int32)
    return rules, offsets


def _classify(per_kind, kinds, charges):
    lib = _abi.load_library()
    rules, offsets = _table(per_kind)
    kinds = np.ascontiguousarray(kinds, dtype=np.int64)
    q = None if charges is None else np.ascontiguousarray(charges, dtype=np.float64)
    consts = np.full(4, np.nan)
    rc = lib.ceg_uniform_class(_abi.i64ptr(kinds), _abi.dptr(q) if q is not None else None, len(kinds), rules.ctypes.data,
                               _abi.i32ptr(offsets), len(per_kind), CUTOFF2, _abi.dptr(consts))
    return rc, consts


O_RULE = (LJ, 107.69, 3.15, 0.0, -0.1375)


def test_one_kind():
    rc, c = _classify([[O_RULE]], [1, 1, 1], [-0.4, -0.4, -0.4])
    assert rc == 2
    assert c[0] == 4.0 * 107.69 and c[1] == (3.15 * 3.15) * (3.15 * 3.15) * (3.15 * 3.15) and c[2] == -0.1375 and c[3] == -0.4
    # no charges given: the Lennard-Jones constants alone
    rc, c = _classify([[O_RULE]], [1, 1, 1], None)
    assert rc == 1 and c[3] == 0.0


def test_two_kinds_with_equal_records():
    rc, c = _classify([[O_RULE], [O_RULE]], [1, 2, 2, 1], [-0.4] * 4)
    assert rc == 2 and c[0] == 4.0 * 107.69


def test_two_kinds_with_different_sigma():
    other = (LJ, 107.69, np.nextafter(3.15, 4.0), 0.0, -0.1375)
    rc, c = _classify([[O_RULE], [other]], [1, 2, 2, 1], [-0.4] * 4)
    assert rc == 0 and np.all(c == 0.0)
    # ... but a kind that does not occur among the atoms does not count
    rc, _ = _classify([[O_RULE], [other]], [1, 1, 1], [-0.4] * 3)
    assert rc == 2
    # a different shift or epsilon breaks it as well
    for other in ((LJ, 107.69, 3.15, 0.0, 0.0), (LJ, np.nextafter(107.69, 200.0), 3.15, 0.0, -0.1375)):
        assert _classify([[O_RULE], [other]], [1, 2], [-0.4] * 2)[0] == 0


def test_equal_lj_one_charge_changed_in_the_last_bit():
    q = np.full(5, -0.4)
    q[3] = np.nextafter(-0.4, 0.0)
    rc, c = _classify([[O_RULE], [O_RULE]], [1, 2, 2, 1, 1], q)
    assert rc == 1 and c[0] == 4.0 * 107.69 and c[3] == 0.0
    # +0.0 and -0.0 are not bit-identical either; and a zero charge cannot be divided out
    assert _classify([[O_RULE]], [1, 1], [0.0, -0.0])[0] == 1
    assert _classify([[O_RULE]], [1, 1], [0.0, 0.0])[0] == 1


def test_a_kind_without_a_rule():
    # kind 2 (Si) has no rule with the probe, kind 3 a NoInteraction rule (dropped at conversion): their atoms are Coulomb-only
    # candidates with charges of their own and do not take part in either test
    per_kind = [[O_RULE], [], [(NONE, 0.0, 0.0, 0.0, 0.0)]]
    rc, c = _classify(per_kind, [1, 2, 3, 1, 2], [-0.4, 0.8, 1.1, -0.4, 0.7])
    assert rc == 2 and c[3] == -0.4
    # nothing VdW-active at all: nothing to defer
    assert _classify(per_kind, [2, 3], [0.8, 1.1])[0] == 0


def test_other_rule_classes_do_not_qualify():
    buck = (BUCK, 5.581e7, 3.985, 9.167e5, 0.0)
    assert _classify([[buck]], [1, 1], [-0.4] * 2)[0] == 0                       # one Buckingham class: VDWK 3, not this
    assert _classify([[O_RULE, O_RULE]], [1, 1], [-0.4] * 2)[0] == 0             # a sum of two rules on one kind
    assert _classify([[(LJ, 0.0, 3.15, 0.0, 0.0)]], [1, 1], [-0.4] * 2)[0] == 0  # epsilon = 0 cannot be divided out


def test_bad_arguments():
    lib = _abi.load_library()
    assert lib.ceg_uniform_class(None, None, 0, None, None, 0, CUTOFF2, None) == -1
    rules, offsets = _table([[O_RULE]])
    kinds = np.array([2], dtype=np.int64)
    assert lib.ceg_uniform_class(_abi.i64ptr(kinds), None, 1, rules.ctypes.data, _abi.i32ptr(offsets), 1, CUTOFF2, None) == -1
    assert lib.ceg_plan_uniform_class(None) == 0
