"""The host restatement of the group sampler (ceg_hip.mcrng: bin_index, bin_positions, sampler_frames, replay_positions) on cases
worked out by hand: the index rule of bin_trajectory (averageclusters.jl:182-188) at its edges, the frames of a sweep at theirs, and a
chain followed through a log written by hand.  No device needed; tests/test_gpu_mc_sampler.py holds the device to this module."""
import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi, mcrng

FF = "BoulfelfelSholl2021"
EYE = np.eye(3)


def test_bin_index_edges_on_a_cubic_cell():
    # u == 0 gives index 0 (ceil(0) + 1 - 1), also for a lattice point several cells away
    assert mcrng.bin_index(EYE, (4, 5, 6), [0.0, 0.0, 0.0]).tolist() == [0, 0, 0]
    assert mcrng.bin_index(EYE, (4, 5, 6), [3.0, -2.0, 7.0]).tolist() == [0, 0, 0]
    # u n an exact integer m gives m - 1: the upper edge of a bin belongs to it (n = 4: u = 1/4, 1/2, 3/4 -> 0, 1, 2)
    assert mcrng.bin_index(EYE, (4, 4, 4), [0.25, 0.5, 0.75]).tolist() == [0, 1, 2]
    # just above an edge: the next bin
    assert mcrng.bin_index(EYE, (4, 4, 4), [0.25 + 2.0 ** -50, 0.5 + 2.0 ** -50, 0.75 + 2.0 ** -50]).tolist() == [1, 2, 3]
    # y = -1e-20: floor is -1 and y + 1 rounds to 1.0, so u n = n and the index is n - 1 (the clamp is not what gives it)
    assert -1e-20 - np.floor(-1e-20) == 1.0
    assert mcrng.bin_index(EYE, (4, 5, 6), [-1e-20, -1e-20, -1e-20]).tolist() == [3, 4, 5]
    # several lattice vectors outside, cell of 8 A, 8 bins: 42.5 = 5 * 8 + 2.5 -> u n = 2.5 -> 2; -21.25 = -3 * 8 + 2.75 -> 2; 7.0 -> 7 - 1 = 6
    assert mcrng.bin_index(EYE / 8.0, (8, 8, 8), [42.5, -21.25, 7.0]).tolist() == [2, 2, 6]
    # vectorised over leading axes
    p = np.array([[[0.0, 0.0, 0.0], [0.25, 0.5, 0.75]]])
    assert mcrng.bin_index(EYE, (4, 4, 4), p).tolist() == [[[0, 0, 0], [0, 1, 2]]]


def test_bin_index_is_evaluated_left_to_right():
    """y_r = (I[r,0] p_x + I[r,1] p_y) + I[r,2] p_z: with I[0] = (1, 1, 1) and p = (1e16, 1, -1e16) the left-to-right sum is 0 (1e16 + 1
    rounds to 1e16); any other order or a fused multiply-add chain starting elsewhere gives 1 or 2 ulp-level residues."""
    I = np.array([[1.0, 1.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    y = mcrng.fractional(I, [1e16, 1.0, -1e16])
    assert y[0] == 0.0
    assert mcrng.bin_index(I, (10, 1, 1), [1e16, 1.0, -1e16])[0] == 0


@pytest.mark.parametrize("name,supercell", [("CHA_1.4_3b4eeb96_Na_11812", (1, 1, 1)), ("CIT-7", (2, 3, 3))])
def test_bin_index_on_the_fixture_cells(name, supercell):
    """The triclinic CHA cell, and the CIT-7 2x3x3 MC cell folded onto its unit cell: a point built as unit_cell @ (bin centre + whole
    lattice vectors) falls into the bin it was built for (a centre is half a bin away from every edge: rounding cannot move it)."""
    unit_true = np.asarray(ceg.load_framework_RASPA(name, FF).mat, dtype=np.float64)
    mc_cell = unit_true * np.asarray(supercell, dtype=np.float64)[None, :]
    unit = mc_cell / np.asarray(supercell, dtype=np.float64)[None, :]              # as set_sampler derives it
    inv = np.linalg.inv(unit)
    assert abs(unit[1, 0]) + abs(unit[0, 1]) + abs(unit[0, 2]) > 0.1                # triclinic: off-diagonal entries
    dims = np.floor(np.linalg.norm(unit, axis=0) / 1.0).astype(int)                 # 1 A bins
    rng = np.random.default_rng(11)
    want = np.stack([rng.integers(0, d, 200) for d in dims], axis=1)
    shifts = np.stack([rng.integers(0, s, 200) for s in supercell], axis=1)          # images inside the MC cell
    far = rng.integers(-3, 4, (200, 3)) * np.asarray(supercell)[None, :]            # and whole MC cells away
    frac = (want + 0.5) / dims[None, :] + shifts + far
    pts = frac @ unit.T
    assert np.array_equal(mcrng.bin_index(inv, dims, pts), want)
    # the images land in every unit cell of the supercell
    assert len({tuple(s) for s in shifts}) == int(np.prod(supercell))


def test_bin_positions_with_a_symmetry_operation():
    """One operation with a translation of 1/3: R a cyclic permutation (y' = (y_1, y_2, y_0) + 1/3), cubic cell, 6 bins per axis.
    p = (0.55, 0.1, 0.9): as it is u n = (3.3, 0.6, 5.4) -> (3, 0, 5); its image (0.1, 0.9, 0.55) + 1/3 = (0.4333, 1.2333, 0.8833) ->
    u n = (2.6, 1.4, 5.3) -> (2, 1, 5).  bins are [c][b][a]."""
    R = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    t = np.full(3, 1.0 / 3.0)
    bins = np.zeros((6, 6, 6), dtype=np.int64)
    out = mcrng.bin_positions(bins, EYE, [[0.55, 0.1, 0.9]], symmetries=[(R, t)])
    assert out is bins and bins.sum() == 2
    assert bins[5, 0, 3] == 1 and bins[5, 1, 2] == 1
    # the same operation as a [3, 4] block, accumulated on top; two atoms in one bin count twice
    mcrng.bin_positions(bins, EYE, [[0.55, 0.1, 0.9], [0.56, 0.11, 0.91]], symmetries=[np.concatenate([R, t[:, None]], axis=1)])
    assert bins.sum() == 6 and bins[5, 0, 3] == 3 and bins[5, 1, 2] == 3
    # the operation acts on the UNFLOORED coordinates: p + (4, 0, 0) has y_0 = 4.55, and the image takes y_0 into its third row
    b2 = np.zeros((6, 6, 6), dtype=np.int64)
    mcrng.bin_positions(b2, EYE, [[4.55, 0.1, 0.9]], symmetries=[(R, t)])
    assert b2[5, 0, 3] == 1 and b2[5, 1, 2] == 1
    # non-cubic shape: (na, nb, nc) = (2, 3, 4) -> array [4, 3, 2]
    b3 = np.zeros((4, 3, 2), dtype=np.int64)
    mcrng.bin_positions(b3, EYE, [[0.9, 0.5, 0.1]])
    assert b3[0, 1, 1] == 1 and b3.sum() == 1


def test_sampler_frames_edges():
    # a frame after step s iff s >= from_step and (s + 1) % every == 0
    assert mcrng.sampler_frames(0, 10, 5) == [4, 9]
    assert mcrng.sampler_frames(0, 10, 5, from_step=5) == [9]                       # from_step inside the window
    assert mcrng.sampler_frames(0, 10, 5, from_step=4) == [4, 9]                    # ... exactly on a frame step
    assert mcrng.sampler_frames(0, 10, 5, from_step=10) == []
    assert mcrng.sampler_frames(5, 99, 8, from_step=16) == [23 + 8 * i for i in range(11)]     # first_step no multiple of every; ends on a frame
    assert mcrng.sampler_frames(5, 96, 8, from_step=16)[-1] == 95
    assert mcrng.sampler_frames(3, 4, 50) == []                                     # every larger than nsteps, no multiple inside
    assert mcrng.sampler_frames(47, 4, 50) == [49]                                  # ... one inside
    assert mcrng.sampler_frames(7, 3, 1) == [7, 8, 9]                               # every = 1
    assert mcrng.sampler_frames(7, 3, 1, from_step=9) == [9]
    assert mcrng.sampler_frames(2 ** 32 - 2, 4, 2) == [2 ** 32 - 1, 2 ** 32 + 1]    # across the low word of the step counter
    assert mcrng.sampler_frames(0, 0, 1) == []
    with pytest.raises(ValueError):
        mcrng.sampler_frames(0, 10, 0)
    for first, n, every, start in ((0, 40, 7, 3), (13, 29, 4, 20), (5, 1, 6, 0)):                 # against the definition
        assert mcrng.sampler_frames(first, n, every, start) == [s for s in range(first, first + n) if s >= start and (s + 1) % every == 0]


def _record(species, molecule, kind, accepted, positions=()):
    r = np.zeros((), dtype=_abi.GCMC_RECORD_DTYPE)
    r["species"], r["molecule"], r["kind"], r["accepted"] = species, molecule, kind, accepted
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    r["positions"][:len(p)] = p
    return r


def test_replay_positions_on_a_log_written_by_hand():
    """Species 0: one atom, species 1: three atoms.  Start: molecules [A(0), B(1), C(0)].  Six accepted records, one per kind the
    device applies differently: translation, rotation, random_reinsertion replace; an insertion appends; a deletion of molecule 0 moves
    the last molecule into the hole; a deletion of the last molecule just drops it."""
    A, C0 = np.array([[1.0, 2.0, 3.0]]), np.array([[7.0, 8.0, 9.0]])
    B = np.arange(9.0).reshape(3, 3)
    B2, B3, A2 = B + 10.0, B + 20.0, A + 0.5
    D = np.arange(9.0).reshape(3, 3) + 100.0
    log = np.array([_record(0, 0, 0, 1, A2),            # translation of A
                    _record(1, 1, 1, 1, B2),            # rotation of B
                    _record(1, 1, 4, 1, B3),            # random_reinsertion of B
                    _record(1, 3, 5, 1, D),             # insertion: D becomes molecule 3
                    _record(0, 0, 6, 1),                # deletion of molecule 0: D moves into index 0
                    _record(0, 2, 6, 1)])               # deletion of the last molecule (C)
    want = [[A2, B, C0], [A2, B2, C0], [A2, B3, C0], [A2, B3, C0, D], [D, B3, C0], [D, B3]]
    want_species = [[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0, 1], [1, 1, 0], [1, 1]]
    got = list(mcrng.replay_positions([A, B, C0], log, [1, 3]))
    assert len(got) == 6
    for g, w in zip(got, want):
        assert len(g) == len(w) and all(np.array_equal(x, y) for x, y in zip(g, w))
    both = list(mcrng.replay_positions([A, B, C0], log, [1, 3], start_species=[0, 1, 0]))
    assert [s for s, _p in both] == want_species
    assert all(np.array_equal(x, y) for (_s, g), w in zip(both, want) for x, y in zip(g, w))
    # the start is not written to
    assert np.array_equal(A, [[1.0, 2.0, 3.0]]) and np.array_equal(B, np.arange(9.0).reshape(3, 3))
    # rejected, spent and blocked records change nothing; the unused tail of a record's positions is not taken
    quiet = np.array([_record(0, 0, 0, 0, A2), _record(1, -1, 6, 0), _record(1, 1, 2, 0, B2)])
    for g in mcrng.replay_positions([A, B, C0], quiet, [1, 3]):
        assert all(np.array_equal(x, y) for x, y in zip(g, [A, B, C0]))
    # a plain sweep's log (no species, kinds 0 and 1)
    plain = np.zeros(2, dtype=_abi.SWEEP_RECORD_DTYPE)
    plain[0]["molecule"], plain[0]["kind"], plain[0]["accepted"] = 1, 1, 1
    plain[0]["positions"][:3] = B2
    plain[1]["molecule"], plain[1]["kind"], plain[1]["accepted"] = 2, 0, 0
    got = list(mcrng.replay_positions([A, B, C0], plain))
    assert np.array_equal(got[0][1], B2) and np.array_equal(got[1][1], B2) and np.array_equal(got[1][2], C0) and got[1][1].shape == (3, 3)


def test_sampler_bindings_restate_the_header_layouts():
    assert _abi.MC_SAMPLE_RECORD_DTYPE.itemsize == 64 and _abi.MC_SAMPLE_RECORD_DTYPE.fields["delta_moves"][1] == 48
    assert _abi.MC_SAMPLER.unit_invmat.offset == 56 and _abi.MC_SAMPLER.chain_map.offset == 128
    assert {"ceg_mc_group_set_sampler", "ceg_mc_group_sample", "ceg_mc_group_sampler_read", "ceg_mc_group_sampler_reset"} <= set(_abi.PROTOTYPES)
