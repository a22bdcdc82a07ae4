"""Block pockets of the GCMC sweeps on the host (no device): ceg_hip.mcrng.block_lookup against hand-built masks, the attempt stream
of the retried proposals, and the per-kind rules of choose_step! (src/simulation.jl:271-326) in mcrng.propose_gcmc(..., blocks=...)."""
from types import SimpleNamespace

import numpy as np
import pytest

from ceg_hip import mcrng
from ceg_hip.hostmirror.coordinates import CellMatrix, GridCoordinatesSetup

SEED = 0x5EED0123456789AB
TRICLINIC = np.array([[10.0, 2.0, 1.0], [0.0, 9.0, 1.5], [0.0, 0.0, 8.0]])          # cell vectors as columns


def _cset():
    return GridCoordinatesSetup.from_cell(CellMatrix.from_mat(TRICLINIC), 0.5)


def _lookup(mask, cs, point, offset=(0.0, 0.0, 0.0)):
    return mcrng.block_lookup(mask, cs.dims, cs.size, cs.shift, offset, cs.cell.mat, cs.cell.invmat, point)


def _index_coordinate(cs, point):
    """0-based lattice coordinate of a point INSIDE the cell (no wrapping)"""
    return (np.asarray(point) - cs.shift) * cs.dims / cs.size


def _point_at(cs, base, axis, target):
    """`base` moved along the cartesian axis so that its lattice coordinate on that axis is `target`"""
    p = np.array(base, dtype=np.float64)
    p[axis] += (target - _index_coordinate(cs, p)[axis]) * cs.size[axis] / cs.dims[axis]
    return p


def test_block_lookup_rounds_to_the_nearest_lattice_point_in_a_triclinic_cell():
    cs = _cset()
    assert np.count_nonzero(TRICLINIC - np.diag(np.diag(TRICLINIC))) == 3
    base = TRICLINIC @ np.array([0.41, 0.37, 0.52])                                 # well inside the cell
    near = np.rint(_index_coordinate(cs, base)).astype(int)
    for axis in range(3):
        i = int(near[axis])
        mask = np.zeros(tuple(int(d) + 1 for d in cs.dims), dtype=bool)
        idx = list(near)
        idx[axis] = i + 1
        mask[tuple(idx)] = True                                                     # the one blocked lattice point: i + 1 on this axis
        below, above = _point_at(cs, base, axis, i + 0.5 - 1e-9), _point_at(cs, base, axis, i + 0.5 + 1e-9)
        assert not _lookup(mask, cs, below) and _lookup(mask, cs, above), axis
        # the far side of the blocked point
        assert _lookup(mask, cs, _point_at(cs, base, axis, i + 1.5 - 1e-9)) and not _lookup(mask, cs, _point_at(cs, base, axis, i + 1.5 + 1e-9)), axis
        # the offset of the atom blocks, delta / 2: a quarter above i belongs to i, and to i + 1 once the offset is added
        quarter = _point_at(cs, base, axis, i + 0.25)
        half = (cs.size / cs.dims) / 2.0
        only = np.zeros(3)
        only[axis] = half[axis]
        assert not _lookup(mask, cs, quarter) and _lookup(mask, cs, quarter, only), axis
        # a point outside the cell is wrapped into it
        for lattice in ((1, 0, 0), (0, -2, 0), (3, 1, -1)):
            moved = above + TRICLINIC @ np.array(lattice, dtype=np.float64)
            assert _lookup(mask, cs, moved) and not _lookup(mask, cs, below + TRICLINIC @ np.array(lattice, dtype=np.float64)), (axis, lattice)
    # the whole offset vector: a quarter above `near` on every axis, the blocked point one up on every axis
    corner = base
    for axis in range(3):
        corner = _point_at(cs, corner, axis, near[axis] + 0.25)
    mask = np.zeros(tuple(int(d) + 1 for d in cs.dims), dtype=bool)
    mask[tuple(near + 1)] = True
    assert not _lookup(mask, cs, corner) and _lookup(mask, cs, corner, (cs.size / cs.dims) / 2.0)


def test_block_lookup_ties_go_to_the_even_index_and_a_null_mask_is_empty():
    # a cell in which every operation of the lookup is exact: 8 A cube, 8 intervals, so the lattice coordinate of x is x itself
    dims, size, shift, zero = (8, 8, 8), (8.0, 8.0, 8.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    mat, invmat = 8.0 * np.eye(3), np.eye(3) / 8.0
    mask = np.zeros((9, 9, 9), dtype=bool)
    mask[3, 3, 4] = True

    def at(x):
        return mcrng.block_lookup(mask, dims, size, shift, zero, mat, invmat, (x, 3.0, 4.0))

    # 1-based coordinate x + 1: 3.5 -> 4 and 4.5 -> 4 (even), 2.5 -> 2 and 5.5 -> 6
    assert at(2.5) and at(3.5) and at(3.0)
    assert not at(1.5) and not at(4.5) and not at(2.5 - 1e-9) and not at(3.5 + 1e-9)
    assert at(2.5 + 8.0) and at(3.5 - 16.0)                                          # wrapped, still exact
    assert mcrng.block_lookup(None, dims, size, shift, zero, mat, invmat, (3.0, 3.0, 4.0)) is False
    # the index is clamped for memory safety only: the last lattice point exists
    mask[:] = False
    mask[8, 8, 8] = True
    assert mcrng.block_lookup(mask, dims, size, shift, zero, mat, invmat, (7.75, 7.75, 7.75))


def test_blocks_object_agrees_with_the_blockfile_of_the_grids_module():
    """mcrng.Blocks on a BlockFile against BlockFile.__getitem__ (an independent restatement) on random points of a triclinic cell"""
    from ceg_hip.grids import BlockFile
    cs = _cset()
    rng = np.random.default_rng(5)
    mask = rng.random(tuple(int(d) + 1 for d in cs.dims)) < 0.4
    bf = BlockFile(cs, mask)
    blocks = mcrng.Blocks([bf, None], [bf])
    half = (cs.size / cs.dims) / 2.0
    for p in rng.uniform(-30.0, 30.0, size=(300, 3)):
        assert blocks.species_blocked(0, p) == bf[p]
        assert blocks.atom_blocked(0, p) == bf[p + half]
        assert not blocks.species_blocked(1, p)
    assert not mcrng.Blocks([bf]).atom_blocked(0, np.zeros(3))                       # no atom blocks installed


# ------------------------------------------------------------------ the proposals
MAT = np.array([[25.0, 3.0, 2.0], [0.0, 24.0, 4.0], [0.0, 0.0, 26.0]])
CO2 = np.array([[-1.16, 0.0, 0.0], [0.0, 0.0, 0.0], [1.16, 0.0, 0.0]])
CENTER, RADIUS = MAT @ np.array([0.5, 0.5, 0.5]), 11.5                               # the sphere blocks ~0.41 of the cell


class Sphere:
    """species 0 is blocked inside a sphere (tested analytically, periodic images included through the wrap of the point)"""

    def species_blocked(self, i, point):
        f = np.linalg.solve(MAT, np.asarray(point, dtype=np.float64))
        w = MAT @ (f - np.floor(f))
        return i == 0 and float(np.linalg.norm(w - CENTER)) < RADIUS

    def atom_blocked(self, kind, point):
        return False


class Nowhere:
    def species_blocked(self, i, point):
        return False

    def atom_blocked(self, kind, point):
        return False


def _species(**weights):
    return [mcrng.GcmcSpecies(CO2, 1, mcrng.MoveTable(**weights), (0, 1, 0))]


def _state(rng, n):
    out = []
    for _ in range(n):
        q = rng.normal(size=(3, 3))
        q, _r = np.linalg.qr(q)
        out.append(MAT @ rng.random(3) + CO2 @ q.T)
    return out


def _propose(step, species, positions, blocks):
    return mcrng.propose_gcmc(SEED, step, 3, [0] * len(positions), positions, species, MAT, 0.8, 0.9, 64, blocks)


def test_attempt_zero_is_the_proposal_without_blocks():
    rng = np.random.default_rng(11)
    positions = _state(rng, 5)
    species = _species(translation=1, rotation=1, random_translation=1, random_rotation=1, random_reinsertion=1, swap=2)
    kinds = set()
    for step in range(120):
        a, b = _propose(step, species, positions, None), _propose(step, species, positions, Nowhere())
        assert a[:4] == b[:4] and np.array_equal(a.positions, b.positions) and a[5:] == b[5:]
        assert (b.attempt, b.pocket) == (0, False)
        kinds.add(a.kind)
    assert kinds == set(range(7))


def test_attempt_t_draws_purpose_or_t_shifted_by_eight():
    step, sid = 2 ** 32 + 5, 7
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    for purpose in (6, 7, 8):
        for t in (0, 1, 17, 999):
            assert mcrng.draw_attempt(SEED, step, sid, purpose, t) == mcrng.philox4x32_10((5, 1, sid, purpose | (t << 8)), key)
        assert mcrng.draw_attempt(SEED, step, sid, purpose, 0) == mcrng.draw(SEED, step, sid, purpose)
    # known answer: counter (5, 1, 7, 6 | 1 << 8), key (0x456789AB, 0x5EED0123)
    assert mcrng.draw_attempt(SEED, step, sid, 6, 1) == (0x96F1D752, 0xBAE7F78E, 0xFB7469F1, 0x64CBA3DF)
    for bad in ((5, 1), (9, 1), (6, 1000), (6, -1)):
        with pytest.raises(ValueError):
            mcrng.draw_attempt(SEED, step, sid, *bad)
    # the placement of attempt t is built from those blocks
    pos = CO2 + np.array([3.0, 4.0, 5.0])
    g, h = mcrng.draw_attempt(SEED, step, sid, 6, 4), mcrng.draw_attempt(SEED, step, sid, 7, 4)
    u = [mcrng.uniform(g[0], g[1]) - 0.5, mcrng.uniform(g[2], g[3]) - 0.5, mcrng.uniform(h[0], h[1]) - 0.5]
    r = np.array([(MAT[d, 0] * u[0] + MAT[d, 1] * u[1]) + MAT[d, 2] * u[2] for d in range(3)])
    assert np.array_equal(mcrng.random_placement(SEED, step, sid, mcrng.RANDOM_TRANSLATION, pos, 1, MAT, 4), pos + r)


def test_insertion_retries_on_the_bead_alone():
    blocks, species = Sphere(), _species(swap=1)
    retried = free_bead_in_pocket = 0
    for step in range(400):
        pr = _propose(step, species, [], blocks)
        if pr.kind != mcrng.SWAP_INSERTION:
            assert pr.kind == mcrng.SWAP_DELETION and pr.spent
            continue
        for t in range(pr.attempt):              # every earlier attempt put the bead into the sphere
            assert blocks.species_blocked(0, mcrng.random_placement(SEED, step, 3, 5, CO2, 1, MAT, t)[1]), (step, t)
        placed = mcrng.random_placement(SEED, step, 3, 5, CO2, 1, MAT, pr.attempt)
        assert np.array_equal(pr.positions, placed) and not blocks.species_blocked(0, placed[1])
        assert pr.pocket == any(blocks.species_blocked(0, p) for p in placed)
        retried += pr.attempt > 0
        free_bead_in_pocket += pr.pocket
    assert retried > 20 and free_bead_in_pocket > 0, (retried, free_bead_in_pocket)


@pytest.mark.parametrize("kind,name", [(2, "random_translation"), (4, "random_reinsertion")])
def test_random_translation_and_reinsertion_retry_on_the_whole_molecule(kind, name):
    blocks, species = Sphere(), _species(**{name: 1})
    positions = _state(np.random.default_rng(3), 6)
    retried = bead_free_but_refused = 0
    for step in range(300):
        pr = _propose(step, species, positions, blocks)
        assert pr.kind == kind and not pr.pocket
        pos = positions[pr.molecule]
        for t in range(pr.attempt):
            earlier = mcrng.random_placement(SEED, step, 3, kind, pos, 1, MAT, t)
            inside = [blocks.species_blocked(0, p) for p in earlier]
            assert any(inside), (step, t)
            bead_free_but_refused += not inside[1]
        placed = mcrng.random_placement(SEED, step, 3, kind, pos, 1, MAT, pr.attempt)
        assert np.array_equal(pr.positions, placed) and not any(blocks.species_blocked(0, p) for p in placed)
        retried += pr.attempt > 0
    assert retried > 20 and bead_free_but_refused > 0, (retried, bead_free_but_refused)


@pytest.mark.parametrize("kind,name", [(0, "translation"), (1, "rotation"), (3, "random_rotation")])
def test_translation_rotation_and_random_rotation_are_tested_once(kind, name):
    blocks, species = Sphere(), _species(**{name: 1})
    positions = _state(np.random.default_rng(4), 8)
    pockets = 0
    for step in range(200):
        pr, plain = _propose(step, species, positions, blocks), _propose(step, species, positions, None)
        assert pr.kind == kind and pr.attempt == 0 and np.array_equal(pr.positions, plain.positions)
        assert pr.pocket == any(blocks.species_blocked(0, p) for p in pr.positions)
        pockets += pr.pocket
    assert 0 < pockets < 200, pockets


def test_an_all_ones_species_mask_exhausts_the_retry_loop():
    cs = GridCoordinatesSetup.from_cell(CellMatrix.from_mat(MAT), 1.0)
    full = SimpleNamespace(csetup=cs, block=np.ones(tuple(int(d) + 1 for d in cs.dims), dtype=bool))
    blocks = mcrng.Blocks([full])
    positions = _state(np.random.default_rng(6), 3)
    for name, kinds in (("random_translation", {2}), ("random_reinsertion", {4}), ("swap", {5, 6})):
        seen = set()
        for step in range(6):
            pr = _propose(step, _species(**{name: 1}), positions, blocks)
            assert pr.kind in kinds
            seen.add(pr.kind)
            if pr.kind == mcrng.SWAP_DELETION:
                assert (pr.attempt, pr.pocket) == (0, False)
                continue
            assert (pr.attempt, pr.pocket) == (999, True) and pr.positions.shape == (0, 3) and not pr.spent and not pr.capacity
        assert kinds - {6} <= seen
    for name in ("translation", "rotation", "random_rotation"):
        pr = _propose(0, _species(**{name: 1}), positions, blocks)
        assert (pr.attempt, pr.pocket) == (0, True) and pr.positions.shape == (3, 3)
    # an insertion at the cap is decided before any block is looked at
    pr = mcrng.propose_gcmc(SEED, 1, 3, [0] * 3, positions, _species(swap=1), MAT, 0.8, 0.9, 3, blocks)
    if pr.kind == mcrng.SWAP_INSERTION:
        assert pr.capacity and (pr.attempt, pr.pocket) == (0, False)


def test_setup_fields_and_the_wrapper_know_about_blocks():
    """MonteCarloSetup carries speciesblocks / atomblocks, empty by default; the group wrapper finds out whether a setup has any"""
    import dataclasses
    from ceg_hip import _abi
    from ceg_hip.energy import DeviceMonteCarloGroup
    from ceg_hip.grids import BlockFile
    from ceg_hip.hostmirror.montecarlo import MonteCarloSetup
    fields = {f.name: f for f in dataclasses.fields(MonteCarloSetup)}
    assert fields["speciesblocks"].default_factory() == [] and fields["atomblocks"].default_factory() == []
    assert _abi.MC_BLOCK_DTYPE.itemsize == 240 and _abi.MC_BLOCK_DTYPE.fields["invmat"][1] == 168
    cs = _cset()
    empty, some = BlockFile(cs), BlockFile(cs, np.ones(tuple(int(d) + 1 for d in cs.dims), dtype=bool))
    carries = DeviceMonteCarloGroup._carries_blocks
    assert not carries(SimpleNamespace()) and not carries(SimpleNamespace(speciesblocks=[empty, None], atomblocks=[]))
    assert carries(SimpleNamespace(speciesblocks=[empty, some])) and carries(SimpleNamespace(speciesblocks=[], atomblocks=[None, some]))
