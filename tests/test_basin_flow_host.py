"""``local_basins_host`` / ``decompose_basins_host`` of ``ceg_hip/basins.py`` (the definition: one levelled pass for all starts) against
the literal, queue-based restatements of ``tests/basin_flow_cases.py`` -- on the CPU, no library involved.

With ``as_written=False`` the literal equals the definition set for set.  With ``as_written=True`` (the skip of basins.jl:153 kept)
every basin differs from the definition only inside the set of sole last-level points, and that corner does occur in these cases."""
import numpy as np
import pytest

import basin_flow_cases as FC
from ceg_hip import basins as B

LITERAL = [c for c in FC.basin_cases() if c[4]]


def _ids(cases):
    return [c[0] for c in cases]


def _sets(b):
    return [set(map(tuple, B.basin_points(b, int(i)).tolist())) for i in b.kept]


@pytest.mark.parametrize("case", LITERAL, ids=_ids(LITERAL))
def test_host_form_equals_the_literal_without_the_skip(case):
    name, g, starts, kw, _ = case
    ref = FC.literal_reference(name)
    b = B.local_basins_host(g, starts, **kw)
    assert b.kept.tolist() == ref["kept"]
    assert _sets(b) == ref["basins"]
    want = FC.expected(name)
    for field in ("level", "owner", "nowners", "shared", "size"):
        assert np.array_equal(getattr(b, field), want[field]), field
    assert b.level.dtype == np.int32 and b.owner.dtype == np.int32 and b.nowners.dtype == np.uint8 and b.shared.dtype == np.int32


def test_the_literal_as_written_differs_only_at_sole_last_level_points():
    differing = with_sole = total = 0
    for name, g, starts, kw, _ in LITERAL:
        fixed, raw = FC.literal_reference(name), FC.literal_reference(name, as_written=True)
        assert raw["kept"] == fixed["kept"], name
        soles = {p for p in raw["sole"] if p is not None}
        for want, got, sole in zip(fixed["basins"], raw["basins"], raw["sole"]):
            total += 1
            with_sole += sole is not None
            diff = want ^ got
            differing += bool(diff)
            assert diff <= soles, (name, sorted(diff))
    assert differing >= 1 and with_sole >= differing, (differing, with_sole, total)      # the corner occurs: the statement is not vacuous


@pytest.mark.parametrize("cluster", [0, 1, 3])
@pytest.mark.parametrize("name", ["random-5x7x3", "random-17x9x33", "smooth-17x9x33", "wrap-17x9x33", "random-17x9x33-skip", "random-2x7x3"])
def test_cluster_against_the_literal_clean_cluster(name, cluster):
    _, g, starts, kw, _ = FC.case(name)
    ref = FC.literal_reference(name, cluster=cluster)
    b = B.local_basins_host(g, starts, cluster=cluster, **kw)
    assert b.kept.tolist() == ref["kept"]
    assert _sets(b) == ref["basins"]
    assert b.size[b.kept].tolist() == [len(s) for s in ref["basins"]]
    assert not b.size[np.setdiff1d(np.arange(len(starts)), b.kept)].any()
    if cluster == 3 and name == "random-17x9x33":
        assert len(ref["kept"]) < len(FC.literal_reference(name)["kept"])           # something was merged


@pytest.mark.parametrize("case", LITERAL, ids=_ids(LITERAL))
def test_decompose_against_the_literal(case):
    name, g, starts, kw, _ = case
    ref = FC.literal_reference(name)
    points, nodes = FC.decompose_basins_literal(g.shape, ref["basins"])
    got_points, offsets, owners = B.decompose_basins_host(g, starts, **kw)
    assert [tuple(p) for p in got_points.tolist()] == points
    assert len(offsets) == len(points) + 1 and offsets[0] == 0 and offsets[-1] == len(owners)
    for n, p in enumerate(points):
        assert tuple(owners[offsets[n]:offsets[n + 1]].tolist()) == nodes[p], p


def test_decompose_accepts_basins_and_clusters():
    _, g, starts, kw, _ = FC.case("random-17x9x33")
    b = B.local_basins_host(g, starts, cluster=3)
    ref = FC.literal_reference("random-17x9x33", cluster=3)
    points, nodes = FC.decompose_basins_literal(g.shape, ref["basins"])
    got_points, offsets, owners = B.decompose_basins_host(b)
    assert [tuple(p) for p in got_points.tolist()] == points
    assert all(tuple(owners[offsets[n]:offsets[n + 1]].tolist()) == nodes[p] for n, p in enumerate(points))


@pytest.mark.parametrize("a", [8, 9, 2, 1])
def test_circular_distance_as_written(a):
    """even and odd lengths, both sides of a // 2: the wrapped distance only when min < a // 2 < max, strictly"""
    for m in range(1, a + 1):
        for n in range(1, a + 1):
            want = FC.circular_distance_literal(a, (m, n))
            assert B.circular_distance(a, m, n) == want
            lo, hi = min(m, n), max(m, n)
            assert want == (min(hi - lo, lo - hi + a) if lo < a // 2 < hi else hi - lo)
    if a == 8:
        assert B.circular_distance(8, 1, 8) == 1 and B.circular_distance(8, 4, 8) == 4 and B.circular_distance(8, 5, 8) == 3
        assert B.circular_distance(8, 1, 4) == 3 and B.circular_distance(8, 3, 8) == 3
    if a == 9:
        assert B.circular_distance(9, 1, 9) == 1 and B.circular_distance(9, 4, 9) == 5 and B.circular_distance(9, 3, 9) == 3


def test_host_refusals():
    _, g, starts, kw, _ = FC.case("random-5x7x3")
    with pytest.raises(ValueError, match="repeats"):
        B.local_basins_host(g, list(starts) + [starts[0]])
    with pytest.raises(ValueError, match="outside"):
        B.local_basins_host(g, list(starts) + [(5, 0, 0)])


def test_minima_default_and_the_large_case_agree_with_a_levelled_relaxation():
    """the large case has no literal: its host reference is checked here against an independent fixed point -- D by relaxation over
    all points until nothing changes, owners by the pull rule"""
    name, g, starts, kw, _ = FC.case("smooth-70x66x65")
    b = B.local_basins_host(g, starts)
    big = np.int32(2**30)
    D = np.where(b.level == 0, 0, big).astype(np.int32)
    while True:
        new = D
        for axis in range(3):
            for s in (1, -1):
                gu, Du = np.roll(g, s, axis=axis), np.roll(D, s, axis=axis)
                new = np.minimum(new, np.where((gu < g) & (Du < big), Du + 1, big))
        if np.array_equal(new, D):
            break
        D = new
    assert np.array_equal(np.where(D < big, D, -1), b.level)
    small = FC.case("random-5x7x3")
    assert B.local_basins_host(small[1]).size.tolist() == B.local_basins_host(small[1], small[2]).size.tolist()
