"""The random stream and the proposals of the Monte-Carlo sweeps as ceg_hip.mcrng restates them (no device): Philox4x32-10 known
answers (the table of include/ceg_hip.h), the uniform construction, and the moves of random_translation / random_rotation
(src/mcmoves.jl:139-164)."""
import math

import numpy as np
import pytest

from ceg_hip import mcrng


def _words(text):
    return tuple(int(w, 16) for w in text.split())


@pytest.mark.parametrize("counter, key, expected", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expected):
    assert mcrng.philox4x32_10(_words(counter), _words(key)) == _words(expected)


def test_draw_lays_out_counter_and_key():
    """key = (seed low, seed high), counter = (step low, step high, stream, purpose)"""
    seed, step = 0x299f31d0a4093822, 0x85a308d3243f6a88
    assert mcrng.draw(seed, step, 0x13198a2e, 0x03707344) == _words("d16cfe09 94fdcceb 5001e420 24126ea1")


def test_uniform_end_points():
    assert mcrng.uniform(0, 0) == 0.0
    assert mcrng.uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert mcrng.uniform(0x80000000, 0) == 0.5
    assert mcrng.uniform(0, 0x7ff) == 0.0            # the low 11 bits of the second word are dropped
    assert mcrng.uniform(0, 0x800) == 2.0 ** -53


CO2 = np.array([[0.0, 0.0, 1.149], [0.0, 0.0, 0.0], [0.0, 0.0, -1.149]])


def _molecules(rng):
    """Na, CO2, a bent three-atom molecule, CO2 again: anywhere in a 20 A box"""
    bent = np.array([[0.0, 0.0, 0.0], [0.9, 0.3, 0.0], [-0.2, 0.8, 0.5]])
    return [rng.uniform(0, 20, (1, 3)), CO2 + rng.uniform(0, 20, 3), bent + rng.uniform(0, 20, 3), CO2 + rng.uniform(0, 20, 3)]


def _distances(p):
    return np.linalg.norm(p[:, None, :] - p[None, :, :], axis=2)


def test_translation_moves_all_atoms_by_one_vector():
    mols = _molecules(np.random.default_rng(3))
    dmax, seen = 0.7, 0
    for step in range(400):
        pr = mcrng.propose(11, step, 5, mols, dmax, 1.0, 0.0, [0, 1, 0, 1])           # p_rotation = 0: translations only
        assert pr.kind == mcrng.TRANSLATION and pr.axis == -1
        d = pr.positions - mols[pr.molecule]
        assert np.array_equal(pr.positions, mols[pr.molecule] + pr.translation)
        assert np.abs(d - d[0]).max() <= 1e-14
        assert (pr.translation >= -dmax).all() and (pr.translation < dmax).all()
        seen += 1
    assert seen == 400
    # the three components come from (w0, w1), (w2, w3) of purpose 1 and (w0, w1) of purpose 2
    g, h = mcrng.draw(11, 7, 5, mcrng.GEOMETRY_A), mcrng.draw(11, 7, 5, mcrng.GEOMETRY_B)
    r = [(2.0 * mcrng.uniform(a, b) - 1.0) * dmax for a, b in ((g[0], g[1]), (g[2], g[3]), (h[0], h[1]))]
    assert np.array_equal(mcrng.propose(11, 7, 5, mols, dmax, 1.0, 0.0, [0, 1, 0, 1]).translation, r)


def test_rotation_keeps_the_bead_and_all_distances():
    mols = _molecules(np.random.default_rng(4))
    bead = [0, 1, 2, 0]
    thetamax, rotations = 2.5, 0
    for step in range(600):
        pr = mcrng.propose(12, step, 9, mols, 0.5, thetamax, 1.0, bead)                # p_rotation = 1
        old = mols[pr.molecule]
        if len(old) == 1:                                                          # a one-atom molecule never rotates
            assert pr.kind == mcrng.TRANSLATION
            continue
        assert pr.kind == mcrng.ROTATION and pr.axis in (0, 1, 2) and -thetamax <= pr.theta < thetamax
        b = bead[pr.molecule]
        assert np.abs(pr.positions[b] - old[b]).max() <= 1e-12
        assert np.abs(_distances(pr.positions) - _distances(old)).max() <= 1e-12
        moved = pr.positions - old[b]
        assert np.abs(moved[:, pr.axis] - (old - old[b])[:, pr.axis]).max() <= 1e-12      # the coordinate along the axis stays
        rotations += 1
    assert rotations > 300


def test_rotation_matrices_are_those_of_the_reference():
    """SMatrix{3,3}(1, 0, 0, 0, c, s, 0, -s, c) etc. (mcmoves.jl:155-161) are filled column by column"""
    t = 0.3
    s, c = math.sin(t), math.cos(t)
    cols = [(1, 0, 0, 0, c, s, 0, -s, c), (c, 0, -s, 0, 1, 0, s, 0, c), (c, s, 0, -s, c, 0, 0, 0, 1)]
    for axis, col in enumerate(cols):
        assert np.array_equal(mcrng.rotation_matrix(t, axis), np.array(col, dtype=np.float64).reshape(3, 3).T)


def test_a_single_atom_never_rotates_and_an_empty_chain_is_idle():
    na = [np.array([[1.0, 2.0, 3.0]])]
    for step in range(200):
        assert mcrng.propose(1, step, 0, na, 0.3, 3.0, 1.0, [0]).kind == mcrng.TRANSLATION
    idle = mcrng.propose(1, 0, 0, [], 0.3, 3.0, 0.5, [])
    assert idle.molecule == -1 and idle.kind == -1 and idle.positions.shape == (0, 3)
    assert idle.u == mcrng.acceptance_draw(1, 0, 0)


def test_frequencies_of_molecule_axis_and_kind():
    """20 000 draws: every molecule, axis and move kind within 4 sigma of its nominal frequency"""
    n, nmol, p_rot = 20000, 5, 0.3
    mols = [CO2 + np.array([3.0 * j, 0.0, 0.0]) for j in range(nmol)]
    molecule, axis, kind = np.zeros(nmol), np.zeros(3), np.zeros(2)
    for step in range(n):
        pr = mcrng.propose(2024, 10 ** 10 + step, 77, mols, 0.4, 1.0, p_rot, [1] * nmol)
        molecule[pr.molecule] += 1
        kind[pr.kind] += 1
        if pr.kind == mcrng.ROTATION:
            axis[pr.axis] += 1

    def within(count, total, p):
        assert abs(count - total * p) <= 4.0 * math.sqrt(total * p * (1.0 - p)), (count, total, p)

    for j in range(nmol):
        within(molecule[j], n, 1.0 / nmol)
    within(kind[mcrng.ROTATION], n, p_rot)
    within(kind[mcrng.TRANSLATION], n, 1.0 - p_rot)
    nrot = int(kind[mcrng.ROTATION])
    for a in range(3):
        within(axis[a], nrot, 1.0 / 3.0)


def test_streams_and_steps_are_independent_of_each_other():
    mols = _molecules(np.random.default_rng(5))
    a = mcrng.propose(3, 100, 1, mols, 0.5, 1.0, 0.5, [0, 1, 0, 1])
    again = mcrng.propose(3, 100, 1, mols, 0.5, 1.0, 0.5, [0, 1, 0, 1])
    assert a.molecule == again.molecule and a.kind == again.kind and np.array_equal(a.positions, again.positions) and a.u == again.u
    us = {mcrng.acceptance_draw(3, s, c) for s in range(50) for c in range(4)}
    assert len(us) == 200


def test_accept_rule():
    before = np.array([-100.0, -20.0, -30.0, 5.0])
    assert mcrng.accept_rule(before, before - 1.0, 0.999, 300.0)                      # downhill: always
    up = before + np.array([30.0, 0.0, 0.0, 0.0])
    assert mcrng.accept_rule(before, up, 0.9 * math.exp(-0.1), 300.0)
    assert not mcrng.accept_rule(before, up, 1.1 * math.exp(-0.1), 300.0)
    blocked = before.copy(); blocked[0] = 1e100
    assert not mcrng.accept_rule(before, blocked, 0.0, 1e300)
