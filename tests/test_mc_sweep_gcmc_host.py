"""The host side of ceg_mc_group_sweep_gcmc (ceg_hip.mcrng): the move table of MCMoves, the proposal of every move kind, the swap
rule and the new Philox purposes -- and the proposal of ceg_mc_group_sweep, which must not have moved.  Needs no device."""
import math

import numpy as np
import pytest

from ceg_hip import mcrng

SEED = 0x5EED0123456789AB
CO2 = np.array([[0.0, 0.0, 0.0], [1.16, 0.0, 0.0], [-1.16, 0.0, 0.0]])
MAT = np.array([[24.0, 1.0, 2.0], [0.0, 25.0, 3.0], [0.0, 0.0, 26.0]])


def test_move_table_reproduces_mcmoves():
    """MCMoves(true), MCMoves(false) (mcmoves.jl:62-68) and the docstring's keyword example (:35-36)"""
    assert mcrng.MoveTable(True).cumulatives == (0.5, 0.5, 1.0, 1.0, 1.0)
    assert mcrng.MoveTable(False).cumulatives == (0.33, 0.66, 0.66, 0.66, 1.0)
    t = mcrng.MoveTable(translation=2, random_rotation=0.5, random_reinsertion=2.5)
    assert t.cumulatives == (2 / 5, 2 / 5, 2 / 5, 2 / 5 + 0.5 / 5, 2 / 5 + 0.5 / 5 + 2.5 / 5)
    assert t["translation"] == 0.4 and abs(t["random_rotation"] - 0.1) < 1e-15 and abs(t["random_reinsertion"] - 0.5) < 1e-15
    assert abs(t.swap) < 1e-15
    s = mcrng.MoveTable(translation=1, swap=1)
    assert s.cumulatives == (0.5,) * 5 and s.swap == 0.5
    # the sampling rule of (m::MCMoves)(r): the first cumulative above r, else swap
    assert [s(r) for r in (0.0, 0.49, 0.5, 0.99)] == [0, 0, 5, 5]
    assert [mcrng.MoveTable(False)(r) for r in (0.0, 0.33, 0.65, 0.66, 0.999)] == [0, 1, 1, 4, 4]
    assert [mcrng.MoveTable(True)(r) for r in (0.2, 0.5, 0.9)] == [0, 2, 2]
    with pytest.raises(ValueError):
        mcrng.MoveTable(translatoin=1)
    with pytest.raises(ValueError):
        mcrng.MoveTable(cumulatives=(0.5, 0.4, 0.6, 0.7, 1.0))


def test_propose_gcmc_kind_frequencies():
    """20 000 steps of one stream: every kind's frequency within 4 binomial standard deviations of the table (species chosen
    uniformly, swaps split evenly)"""
    species = [mcrng.GcmcSpecies(CO2[:1], 0, mcrng.MoveTable(translation=1, random_translation=1, swap=2)),
               mcrng.GcmcSpecies(CO2, 0, mcrng.MoveTable(translation=1, rotation=1, random_translation=1, random_rotation=1,
                                                         random_reinsertion=1, swap=3))]
    spec_of = [0, 1, 1, 0, 1]
    pos = [CO2[:1] + 1.0, CO2 + 2.0, CO2 + 5.0, CO2[:1] - 3.0, CO2 - 7.0]
    n = 20000
    counts = np.zeros((2, 7))
    chosen = np.zeros(5)
    for s in range(n):
        p = mcrng.propose_gcmc(SEED, s, 3, spec_of, pos, species, MAT, 0.5, 1.0)
        counts[p.species, p.kind] += 1
        assert not p.spent and not p.capacity
        assert p.n_species == spec_of.count(p.species)
        if p.kind == mcrng.SWAP_INSERTION:
            assert p.molecule == 5 and p.positions.shape == (len(species[p.species].model), 3)
        else:
            assert spec_of[p.molecule] == p.species
            chosen[p.molecule] += 1
            assert p.positions.shape == ((0, 3) if p.kind == mcrng.SWAP_DELETION else pos[p.molecule].shape)
    for i, sp in enumerate(species):
        for kind in range(7):
            prob = 0.5 * (sp.moves[mcrng.MOVE_NAMES[kind]] if kind < 5 else 0.5 * sp.moves.swap)
            sd = math.sqrt(n * prob * (1.0 - prob))
            assert abs(counts[i, kind] - n * prob) <= 4.0 * sd, (i, kind, counts[i, kind], n * prob, sd)
    # the molecule of a species is uniform among its members
    for members in ([0, 3], [1, 2, 4]):
        tot = chosen[members].sum()
        prob = 1.0 / len(members)
        for d in members:
            assert abs(chosen[d] - tot * prob) <= 4.0 * math.sqrt(tot * prob * (1.0 - prob)), (d, chosen)


def test_propose_gcmc_geometry():
    """Every kind keeps the molecule rigid; translations move every atom alike; rotations keep the bead; a random translation lies in
    the cell's parallelepiped about the start; an insertion is the moved model; spent steps and the capacity limit are flagged."""
    species = [mcrng.GcmcSpecies(CO2[:1], 0, mcrng.MoveTable(random_rotation=1, rotation=1, swap=1)),
               mcrng.GcmcSpecies(CO2, 1, mcrng.MoveTable(translation=1, rotation=1, random_translation=1, random_rotation=1,
                                                         random_reinsertion=1, swap=2))]
    spec_of, pos = [1, 0, 1], [CO2 + 3.0, CO2[:1] + 1.0, CO2 - 4.0]
    seen = set()

    def dist(x):
        return np.linalg.norm(x[:, None] - x[None], axis=2)

    for s in range(400):
        p = mcrng.propose_gcmc(SEED + 1, s, 0, spec_of, pos, species, MAT, 0.5, 1.0)
        seen.add((p.species, p.kind))
        if p.kind == mcrng.SWAP_DELETION:
            continue
        old = species[p.species].model if p.kind == mcrng.SWAP_INSERTION else pos[p.molecule]
        assert np.abs(dist(p.positions) - dist(old)).max() < 1e-12
        bead = species[p.species].bead
        if p.kind in (mcrng.ROTATION, mcrng.RANDOM_ROTATION):
            assert np.array_equal(p.positions[bead], old[bead])
            if len(old) == 1:
                assert np.array_equal(p.positions, old)                    # a rotation of one atom is the identity
        if p.kind in (mcrng.TRANSLATION, mcrng.RANDOM_TRANSLATION):
            d = p.positions - old
            assert np.abs(d - d[0]).max() < 1e-12
            if p.kind == mcrng.TRANSLATION:
                assert np.abs(d).max() <= 0.5
        if p.kind in (mcrng.RANDOM_TRANSLATION, mcrng.RANDOM_REINSERTION, mcrng.SWAP_INSERTION):
            f = np.linalg.solve(MAT, p.positions[bead] - old[bead])
            assert np.abs(f).max() <= 0.5 + 1e-12
            assert np.allclose(p.positions[bead] - old[bead], mcrng.random_translation_vector(SEED + 1, s, 0, MAT), rtol=0, atol=1e-12)
    assert len(seen) == 4 + 7, seen
    # spent: no molecule of the species and not an insertion; the capacity limit
    spent = [mcrng.propose_gcmc(SEED + 1, s, 0, [], [], species, MAT, 0.5, 1.0) for s in range(200)]
    assert any(p.spent for p in spent) and any(p.kind == mcrng.SWAP_INSERTION for p in spent)
    for p in spent:
        assert p.spent == (p.kind != mcrng.SWAP_INSERTION) and (p.molecule == -1) == p.spent and p.n_species == 0
    full = [mcrng.propose_gcmc(SEED + 1, s, 0, spec_of, pos, species, MAT, 0.5, 1.0, max_molecules=3) for s in range(200)]
    assert any(p.capacity for p in full)
    assert all(p.capacity == (p.kind == mcrng.SWAP_INSERTION) for p in full)


def test_swap_rule_hand_computed():
    """compute_accept_move_swap (gcmc.jl:77-88) on numbers worked out by hand"""
    T = 300.0
    # insertion into an empty species: E = 0, self = 0, tc = 0 -> threshold = (phi / T) / 1 = 2
    assert mcrng.swap_threshold([0.0, 0.0, 0.0, 0.0], T, 0, 600.0, 0.0, 0.0, True) == (0.0, 2.0)
    assert mcrng.swap_rule([0.0] * 4, 0.999, T, 0, 600.0, 0.0, 0.0, True)
    # N = 3, diff = (E - self) + tc = (-400 + 100) + 0 = -300 -> threshold = (150 / 300) / 4 * e
    diff, thr = mcrng.swap_threshold([-100.0, -50.0, -200.0, -50.0], T, 3, 150.0, -100.0, 0.0, True)
    assert diff == -300.0 and thr == pytest.approx(0.125 * math.e, rel=1e-15)
    assert mcrng.swap_rule([-100.0, -50.0, -200.0, -50.0], 0.33, T, 3, 150.0, -100.0, 0.0, True)
    assert not mcrng.swap_rule([-100.0, -50.0, -200.0, -50.0], 0.35, T, 3, 150.0, -100.0, 0.0, True)
    # deletion: diff = -(E - self) + tc = 300 + 30 -> threshold = (3 * 300 / 150) exp(-1.1)
    diff, thr = mcrng.swap_threshold([-100.0, -50.0, -200.0, -50.0], T, 3, 150.0, -100.0, 30.0, False)
    assert diff == 330.0 and thr == pytest.approx(6.0 * math.exp(-1.1), rel=1e-15)
    assert mcrng.swap_rule([-100.0, -50.0, -200.0, -50.0], 1.99, T, 3, 150.0, -100.0, 30.0, False)
    assert not mcrng.swap_rule([-100.0, -50.0, -200.0, -50.0], 0.5, T, 3, 1500.0, -100.0, 30.0, False)      # threshold 0.1997
    # a blocked insertion is rejected whatever u; the deletion of a blocked molecule is accepted (threshold inf)
    assert not mcrng.swap_rule([1e100, 0.0, 0.0, 0.0], 0.0, T, 0, 1e300, 0.0, 0.0, True)
    assert mcrng.swap_rule([1e100, 0.0, 0.0, 0.0], 0.999, T, 1, 1.0, 0.0, 0.0, False)
    # the tail-correction change against the host mirror's modify_species_dryrun
    from ceg_hip.hostmirror.montecarlo import modify_species_dryrun
    fw = [1.5, -2.25]
    cross = np.array([[0.5, -0.125], [-0.125, 0.75]])
    for counts in ([0, 0], [3, 1], [0, 7]):
        for i in (0, 1):
            for num in (1, -1):
                assert mcrng.tail_change(fw[i], cross[i], counts, i, num) == modify_species_dryrun(fw, cross, counts, i, num)


def test_philox_known_answers_of_the_new_purposes():
    """draw(seed, step, stream, purpose) for purposes 4-8 at a step beyond 2^32 (Philox4x32-10 itself: tests/test_mc_sweep_host.py)"""
    want = {4: (0x63fdc9ad, 0x33ec173c, 0x19660557, 0xb775aa74), 5: (0xb3640c07, 0x16b3893f, 0xfcb4a3ed, 0xb377d4a7),
            6: (0x453dd54b, 0x37d4ed76, 0xaf9a9aea, 0x99ac0813), 7: (0x7476ef22, 0x93c8578b, 0xfb920e69, 0x6fca0575),
            8: (0x5893f627, 0xd7528814, 0xa617fc9b, 0x1cf748fa)}
    assert (mcrng.GCMC_SELECT, mcrng.GCMC_MOLECULE, mcrng.GCMC_RANDOM_A, mcrng.GCMC_RANDOM_B, mcrng.GCMC_RANDOM_C) == (4, 5, 6, 7, 8)
    for purpose, words in want.items():
        assert tuple(mcrng.draw(SEED, 2 ** 32 + 5, 11, purpose)) == words, purpose
        assert tuple(mcrng.philox4x32_10((5, 1, 11, purpose), (0x456789AB, 0x5EED0123))) == words


def test_the_old_proposal_is_untouched():
    """mcrng.propose on fixed inputs: the values the module gave before propose_gcmc was added"""
    pos = [np.array([[1.0, 2.0, 3.0]]), np.array([[4.0, 5.0, 6.0], [5.16, 5.0, 6.0], [2.84, 5.0, 6.0]]),
           np.array([[-1.5, 0.25, 7.0], [-0.34, 0.25, 7.0], [-2.66, 0.25, 7.0]])]
    want = [
        (0, 0, 0, 0, [[1.0770810239580926, 1.7889605411964267, 3.4940038530616837]], 0.8888032668362728,
         [0.07708102395809258, -0.21103945880357322, 0.4940038530616837], 0.0, -1),
        (7, 3, 2, 0, [[-1.5924417084669298, 0.30994155379990407, 6.629607215936861], [-0.4324417084669298, 0.30994155379990407, 6.629607215936861],
                      [-2.7524417084669297, 0.30994155379990407, 6.629607215936861]], 0.763935819309426,
         [-0.09244170846692978, 0.05994155379990407, -0.370392784063139], 0.0, -1),
        (4294967301, 11, 1, 1, [[4.0, 5.0, 6.0], [5.16, 5.0, 6.0], [2.84, 5.0, 6.0]], 0.5647551599031089, [0.0, 0.0, 0.0], 0.3941296797332181, 0),
        (12345, 2, 1, 0, [[3.6036966561589705, 4.588049968277234, 5.631822078433046], [4.76369665615897, 4.588049968277234, 5.631822078433046],
                          [2.4436966561589704, 4.588049968277234, 5.631822078433046]], 0.3866939973849336,
         [-0.3963033438410295, -0.4119500317227659, -0.3681779215669533], 0.0, -1),
    ]
    for step, sid, molecule, kind, positions, u, translation, theta, axis in want:
        p = mcrng.propose(SEED, step, sid, pos, 0.5, 1.0, 0.5, [0, 0, 0])
        assert (p.molecule, p.kind, p.u, p.theta, p.axis) == (molecule, kind, u, theta, axis)
        assert p.positions.tolist() == positions and p.translation.tolist() == translation
