"""The random stream and the move proposals of the Monte-Carlo sweeps (``ceg_mc_group_sweep``), restated in NumPy.

Needs no device.  The sweep kernels of ``csrc/ceg_mc_sweep.hip`` (through ``csrc/ceg_philox.h``) and this module follow the
specification in ``include/ceg_hip.h`` word for word: Philox4x32-10, one block per (step, stream, purpose), nothing random
stored.  A caller uses it to audit a sweep's log, to replay a chain on the host, or to predict what a chain will propose.

Purposes for stream ``c`` at the absolute step ``s`` (key = seed low / high word, counter = step low, step high, stream, purpose):
  0  selection   molecule ``min(floor(U(w0, w1) nmol), nmol - 1)``; a rotation iff the molecule has more than one atom and
                 ``U(w2, w3) < p_rotation``
  1, 2 geometry  translation (``random_translation``, mcmoves.jl:139-146): ``r = (2U - 1) dmax`` per axis from (w0, w1), (w2, w3)
                 of purpose 1 and (w0, w1) of purpose 2; rotation (``random_rotation``, :147-164): ``theta = thetamax (2 U(w0, w1) - 1)``,
                 axis ``min(floor(3 U(w2, w3)), 2)`` of purpose 1, about atom ``bead``
  3  acceptance  ``u = U(w0, w1)``

``ceg_mc_group_sweep_gcmc`` (all six move kinds of mcmoves.jl:1-8, :func:`propose_gcmc`) keeps purposes 1-3 and adds:
  4  selection   species ``min(floor(U(w0, w1) nspecies), nspecies - 1)``; move kind: the first cumulative of the species'
                 :class:`MoveTable` above ``U(w2, w3)``, else a swap
  5  molecule    ``j = min(floor(U(w0, w1) N_i), N_i - 1)``, the j-th molecule of the species in device molecule order; a swap is a
                 deletion iff ``U(w2, w3) < 0.5``
  6, 7, 8 random_* geometry  ``r = mat (U3 - 0.5)`` with ``U3`` from (w0, w1), (w2, w3) of purpose 6 and (w0, w1) of purpose 7
                 (mcmoves.jl:143); ``theta = pi (2 U(w2, w3) - 1)`` of purpose 7, axis ``min(floor(3 U(w0, w1)), 2)`` of purpose 8

Block pockets (``ceg_mc_group_set_blocks``; ``propose_gcmc(..., blocks=...)``): attempt ``t = 0..999`` of a proposal that ``choose_step!``
retries (simulation.jl:299-320) draws purposes 6-8 with counter word 3 = ``purpose | (t << 8)`` (:func:`draw_attempt`); attempt 0 is the
plain purpose.  :func:`block_lookup` is ``BlockFile`` getindex (coordinates.jl:58-66,97-101) in the device's operation order.

Cycles (``ceg_mc_group_sweep_cycles`` / ``ceg_mc_group_sweep_gcmc_cycles``): :func:`adapt_dmax`, :func:`adapt_thetamax` and
:func:`cycle_records` restate the end-of-cycle adaptation of ``statistics.dmax`` / ``θmax`` (simulation.jl:818-827) in the operation
order of ``k_mcg_cycle_end``, ``thetamax`` in radians.

Tempering (``ceg_mc_group_set_tempering``): purpose 9 is the draw of a replica exchange, ``u = U(w0, w1)`` at the cycle's absolute last
step on the stream of the pair's chain on the lower rung; :func:`exchange_pairs`, :func:`exchange_threshold` and :func:`exchange_round`
restate ``k_mcg_exchange`` (the rule of ``run_parallel_tempering``, simulation.jl:533).

Isotherms (``ceg_mc_group_set_chain_plan``, ``DeviceMonteCarloGroup.make_isotherm``): :func:`isotherm_ncycles`, :func:`accessible_volume`,
:func:`phiPV_div_k` and :meth:`MoveTable.for_gcmc` restate the host arithmetic of ``make_isotherm`` / ``run_gcmc`` / ``GCMCData``
(parameterinputs.jl:274-279,319, gcmc.jl:26-37, simulation.jl:714-715); the fugacity coefficient stays with the caller.

Neighbour cells (``ceg_mc_group_set_device_cells``): :class:`CellBook` restates the cell lists of a chain (``CellMirror`` of
``csrc/ceg_mc_state.h``: ``bin_of``, ``take_out``, ``put_in``, ``refresh``) and :func:`replay_cell_book` follows them through a sweep's log.

Site hopping (``ceg_site_group_sweep_cycles``, ``csrc/ceg_site.hip``): purpose 10 draws the molecule and the site of a hop, purpose 3 the
acceptance; :func:`site_propose`, :func:`site_row_sum` (the device's summation order), :func:`site_movement_energy`, :func:`site_step`
and :func:`site_replay` restate ``k_site_sweep``, :func:`site_baseline` is ``baseline_energy(::SiteHopping)`` in extended precision, and
:func:`site_random_population` (purpose 11, host only) draws the ``randperm`` start of a quench.  The section at the end of this file.
Purpose 12 is the per-step exchange draw of a tempering ladder (``ceg_site_group_set_tempering``, ``k_site_sweep_pt``):
:func:`site_exchange_cdf`, :func:`site_exchange_draw`, :func:`site_exchange_threshold` and :func:`site_ladder_replay`, with the rule
restated above them.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF

SELECT, GEOMETRY_A, GEOMETRY_B, ACCEPT = 0, 1, 2, 3
TRANSLATION, ROTATION = 0, 1
GCMC_SELECT, GCMC_MOLECULE, GCMC_RANDOM_A, GCMC_RANDOM_B, GCMC_RANDOM_C = 4, 5, 6, 7, 8
RANDOM_TRANSLATION, RANDOM_ROTATION, RANDOM_REINSERTION, SWAP_INSERTION, SWAP_DELETION = 2, 3, 4, 5, 6
MOVE_NAMES = ("translation", "rotation", "random_translation", "random_rotation", "random_reinsertion", "swap")      # mcmovenames
KIND_NAMES = MOVE_NAMES[:5] + ("swap_insertion", "swap_deletion")


def philox4x32_10(counter: Sequence[int], key: Sequence[int]):
    """Philox4x32-10: ``counter`` four and ``key`` two 32-bit words -> four 32-bit words."""
    c0, c1, c2, c3 = (int(x) & _MASK for x in counter)
    k0, k1 = (int(x) & _MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + W0) & _MASK, (k1 + W1) & _MASK
    return c0, c1, c2, c3


def uniform(a: int, b: int) -> float:
    """``U(a, b) = ((a << 21) | (b >> 11)) 2^-53`` in [0, 1)."""
    return float(((int(a) & _MASK) << 21) | ((int(b) & _MASK) >> 11)) * 2.0 ** -53


def draw(seed: int, step: int, stream_id: int, purpose: int):
    """The block of (seed, absolute step, stream, purpose)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((step & _MASK, step >> 32, stream_id, purpose), (seed & _MASK, seed >> 32))


ATTEMPTS = 1000           # the retry loop of choose_step! (simulation.jl:299)


def draw_attempt(seed: int, step: int, stream_id: int, purpose: int, attempt: int):
    """The block of attempt ``attempt`` of a retried proposal: purposes 6-8 with counter word 3 = ``purpose | (attempt << 8)``."""
    if not (GCMC_RANDOM_A <= purpose <= GCMC_RANDOM_C and 0 <= attempt < ATTEMPTS):
        raise ValueError("only purposes 6-8 are retried, 1000 times at the most")
    return draw(seed, step, stream_id, purpose | (attempt << 8))


def block_lookup(mask, dims, size, shift, offset, mat, invmat, point) -> bool:
    """``BlockFile`` getindex at ``point + offset`` (coordinates.jl:58-66,97-101), every operation in the order of the device:
    ``wrap_atom`` with the products summed left to right, ``(q - shift) * dims / size + 1``, round to nearest even, the index clamped
    to the mask for memory safety only.  ``mask``: [dims[0]+1, dims[1]+1, dims[2]+1] (None: an empty block, never blocked);
    ``mat`` / ``invmat``: the block's cell with the vectors as columns."""
    if mask is None:
        return False
    M, I = np.asarray(mat, dtype=np.float64), np.asarray(invmat, dtype=np.float64)
    q = [float(point[c]) + float(offset[c]) for c in range(3)]
    abc = [(float(I[r, 0]) * q[0] + float(I[r, 1]) * q[1]) + float(I[r, 2]) * q[2] for r in range(3)]
    abc = [x - math.floor(x) for x in abc]
    w = [(float(M[r, 0]) * abc[0] + float(M[r, 1]) * abc[1]) + float(M[r, 2]) * abc[2] for r in range(3)]
    idx = []
    for c in range(3):
        sh = (w[c] - float(shift[c])) * float(int(dims[c])) / float(size[c]) + 1.0
        idx.append(min(max(int(np.rint(sh)) - 1, 0), int(dims[c])))
    return bool(mask[idx[0], idx[1], idx[2]])


class Blocks:
    """The masks of a chain group as :func:`propose_gcmc` asks for them: ``species[i]`` and ``atoms[kind]`` are objects with ``block``
    (bool[nx, ny, nz] or None) and ``csetup`` (dims, size, shift, cell.mat, cell.invmat) such as ``grids.BlockFile``, or None; ``atoms``
    empty: no atom blocks.  Atom blocks are looked up at ``point + (size / dims) / 2`` (montecarlo.jl:636)."""

    def __init__(self, species, atoms=()):
        self.species, self.atoms = list(species), list(atoms or ())

    @staticmethod
    def _holds(b, point, half: bool) -> bool:
        if b is None or b.block is None or not b.block.any():
            return False
        cs = b.csetup
        offset = [(float(cs.size[c]) / float(int(cs.dims[c]))) / 2.0 if half else 0.0 for c in range(3)]
        return block_lookup(b.block, cs.dims, cs.size, cs.shift, offset, cs.cell.mat, cs.cell.invmat, point)

    def species_blocked(self, i: int, point) -> bool:
        return self._holds(self.species[i], point, False)

    def atom_blocked(self, kind: int, point) -> bool:
        return bool(self.atoms) and self._holds(self.atoms[kind], point, True)


def rotation_matrix(theta: float, axis: int) -> np.ndarray:
    """The three matrices of ``random_rotation`` (mcmoves.jl:155-161; Julia's SMatrix is filled column by column)."""
    s, c = math.sin(theta), math.cos(theta)
    if axis == 0:
        return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    if axis == 1:
        return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


class Proposal(NamedTuple):
    molecule: int             # index into ``positions_of_molecules``; -1: no molecule, the chain is idle
    kind: int                 # TRANSLATION, ROTATION; -1 idle
    positions: np.ndarray     # float64[m, 3] trial placement (empty when idle)
    u: float                  # the acceptance draw of the step
    translation: np.ndarray   # float64[3] (zeros for a rotation)
    theta: float              # radians (0 for a translation)
    axis: int                 # 0, 1, 2 (-1 for a translation)


def acceptance_draw(seed: int, step: int, stream_id: int) -> float:
    w = draw(seed, step, stream_id, ACCEPT)
    return uniform(w[0], w[1])


def propose(seed: int, step: int, stream_id: int, positions_of_molecules, dmax: float, thetamax: float, p_rotation: float,
            bead) -> Proposal:
    """What stream ``stream_id`` proposes at the absolute step ``step`` for a chain whose molecules sit at
    ``positions_of_molecules[j]`` (float64[m_j, 3], device molecule order).  ``thetamax`` in radians; ``bead[j]`` the 0-based
    atom molecule ``j`` rotates about."""
    nmol = len(positions_of_molecules)
    u = acceptance_draw(seed, step, stream_id)
    if nmol == 0:
        return Proposal(-1, -1, np.empty((0, 3)), u, np.zeros(3), 0.0, -1)
    w = draw(seed, step, stream_id, SELECT)
    j = min(int(math.floor(uniform(w[0], w[1]) * nmol)), nmol - 1)
    pos = np.asarray(positions_of_molecules[j], dtype=np.float64).reshape(-1, 3)
    rotate = len(pos) > 1 and uniform(w[2], w[3]) < p_rotation
    g = draw(seed, step, stream_id, GEOMETRY_A)
    if not rotate:
        h = draw(seed, step, stream_id, GEOMETRY_B)
        r = np.array([(2.0 * uniform(g[0], g[1]) - 1.0) * dmax, (2.0 * uniform(g[2], g[3]) - 1.0) * dmax,
                      (2.0 * uniform(h[0], h[1]) - 1.0) * dmax])
        return Proposal(j, TRANSLATION, pos + r, u, r, 0.0, -1)
    theta = thetamax * (2.0 * uniform(g[0], g[1]) - 1.0)
    axis = min(int(math.floor(3.0 * uniform(g[2], g[3]))), 2)
    ref = pos[int(bead[j])]
    new = ref + (pos - ref) @ rotation_matrix(theta, axis).T
    return Proposal(j, ROTATION, new, u, np.zeros(3), theta, axis)


def accept_rule(before, after, u: float, temperature: float) -> bool:
    """``compute_accept_move`` (montecarlo.jl:702-712) on two rows of ``movement_energy`` (framework vdw, framework direct,
    guest-guest, reciprocal; K): rejected when the trial is blocked (framework vdw >= 1e90), accepted when the sum went down,
    else with probability ``exp((b - a) / T)``."""
    if after[0] >= 1e90:
        return False
    b = ((before[0] + before[1]) + before[2]) + before[3]
    a = ((after[0] + after[1]) + after[2]) + after[3]
    return bool(a < b or u < math.exp((b - a) / temperature))


def default_beads(mc):
    """0-based reference atom per kind of a ``MonteCarloSetup``: ``mc.bead`` (1-based, montecarlo.jl:18) when the setup carries it,
    else the atom closest to the mean position of the kind's model (montecarlo.jl:162-177)."""
    given = getattr(mc, "bead", None)
    if given is not None and len(given) == len(mc.ffidx):
        return [int(b) - 1 for b in given]
    out = []
    for i, ids in enumerate(mc.ffidx):
        model = None
        if getattr(mc, "models", None) and i < len(mc.models):
            model = np.asarray(mc.models[i], dtype=np.float64).reshape(-1, 3)
        elif mc.positions[i]:
            model = np.asarray(mc.positions[i][0], dtype=np.float64).reshape(-1, 3)
        if model is None or len(model) != len(ids):
            out.append(0)
            continue
        d2 = ((model - model.mean(axis=0)) ** 2).sum(axis=1)
        out.append(int(np.argmin(d2)))
    return out


# ------------------------------------------------------------------ ceg_mc_group_sweep_gcmc
class MoveTable:
    """``MCMoves`` (mcmoves.jl:58-118): the five cumulative probabilities of translation, rotation, random_translation,
    random_rotation and random_reinsertion; the rest up to 1 is the swap probability.  ``MoveTable(True)`` / ``MoveTable(False)``
    are ``MCMoves(monoatomic)`` (:62-68); ``MoveTable(translation=2, random_rotation=0.5, ...)`` normalises keyword weights like
    ``MCMoves(; ...)`` (:84-95); ``MoveTable(cumulatives=(...))`` takes the tuple as it is."""

    def __init__(self, monoatomic=None, *, cumulatives=None, **weights):
        if cumulatives is not None:
            c = tuple(float(x) for x in cumulatives)
        elif monoatomic is not None:
            c = (0.5, 0.5, 1.0, 1.0, 1.0) if monoatomic else (0.33, 0.66, 0.66, 0.66, 1.0)
        else:
            wrong = [n for n in weights if n not in MOVE_NAMES]
            if wrong:
                raise ValueError(f"invalid move name(s) {wrong}: choose among {MOVE_NAMES}")
            tot = float(sum(weights.values()))
            acc, c = 0.0, []
            for name in MOVE_NAMES[:5]:
                acc += float(weights.get(name, 0.0) / tot)
                c.append(acc)
            c = tuple(c)
        if len(c) != 5 or any(b < a for a, b in zip((0.0,) + c, c)) or c[-1] > 1.0:
            raise ValueError(f"cumulative probabilities must be five non-decreasing values in [0, 1]: {c}")
        self.cumulatives = c

    @property
    def swap(self) -> float:
        return 1.0 - self.cumulatives[-1]

    def __call__(self, r: float) -> int:
        """the move of the draw ``r`` in [0, 1): index into MOVE_NAMES (5: swap)"""
        for k, c in enumerate(self.cumulatives):
            if r < c:
                return k
        return 5

    def for_gcmc(self) -> "MoveTable":
        """The table ``run_gcmc`` runs the first species with (parameterinputs.jl:274-279): a table without swap probability
        (``cumulatives[end] ≈ 1.0``) gets every cumulative before the swap times 2/3, i.e. a swap probability of 1/3; any other is kept."""
        if not math.isclose(self.cumulatives[-1], 1.0, rel_tol=math.sqrt(2.0 ** -52), abs_tol=0.0):
            return self
        return MoveTable(cumulatives=tuple(c * 2 / 3 for c in self.cumulatives))

    def __getitem__(self, name: str) -> float:
        k = MOVE_NAMES.index(name)
        return self.swap if k == 5 else self.cumulatives[k] - (self.cumulatives[k - 1] if k else 0.0)

    def __eq__(self, other):
        return isinstance(other, MoveTable) and self.cumulatives == other.cumulatives

    def __repr__(self):
        return "MoveTable(; " + ", ".join(f"{n}={self[n]:.9g}" for n in MOVE_NAMES if self[n] > 1e-15) + ")"


class GcmcSpecies(NamedTuple):
    model: np.ndarray         # float64[m, 3], mc.models[i]
    bead: int                 # 0-based atom the species rotates about
    moves: MoveTable
    kinds: tuple = ()         # 0-based atom kinds (ff index - 1): what the atom blocks are indexed by


class GcmcProposal(NamedTuple):
    species: int
    kind: int                 # TRANSLATION ... RANDOM_REINSERTION, SWAP_INSERTION, SWAP_DELETION
    molecule: int             # index into ``positions_of_molecules``; an insertion: the index it takes; -1: the step is spent
    n_species: int            # molecules of the species before the move
    positions: np.ndarray     # float64[m, 3] proposed placement (empty for a deletion and a spent step)
    u: float
    spent: bool               # no molecule of the species and not an insertion (simulation.jl:282)
    capacity: bool            # an insertion at max_molecules: counted, not evaluated, rejected
    attempt: int = 0          # with blocks: the attempt the proposal comes from (999 when the retry loop ran out)
    pocket: bool = False      # with blocks: the step is pocket-blocked (positions: the proposal tested, empty when the loop ran out)


def random_translation_vector(seed: int, step: int, stream_id: int, mat, attempt: int = 0) -> np.ndarray:
    """``mat * (rand(SVector{3}) .- 0.5)`` (mcmoves.jl:143), ``mat`` with the cell vectors as columns"""
    g, h = draw_attempt(seed, step, stream_id, GCMC_RANDOM_A, attempt), draw_attempt(seed, step, stream_id, GCMC_RANDOM_B, attempt)
    a, b, c = uniform(g[0], g[1]) - 0.5, uniform(g[2], g[3]) - 0.5, uniform(h[0], h[1]) - 0.5
    M = np.asarray(mat, dtype=np.float64)
    return np.array([(float(M[d, 0]) * a + float(M[d, 1]) * b) + float(M[d, 2]) * c for d in range(3)])


def random_placement(seed: int, step: int, stream_id: int, kind: int, pos, bead: int, mat, attempt: int = 0) -> np.ndarray:
    """Attempt ``attempt`` of the placement a random_* kind or an insertion proposes for a molecule (an insertion: the model) at ``pos``:
    random_translation by ``mat (U3 - 0.5)`` (not for random_rotation), then, unless the kind is random_translation or the molecule
    has one atom, the rotation by ``pi (2U - 1)`` about atom ``bead`` (simulation.jl:294-305)."""
    new = np.array(pos, dtype=np.float64).reshape(-1, 3)
    if kind != RANDOM_ROTATION:
        new = new + random_translation_vector(seed, step, stream_id, mat, attempt)
    if kind != RANDOM_TRANSLATION and len(new) > 1:
        h, k = draw_attempt(seed, step, stream_id, GCMC_RANDOM_B, attempt), draw_attempt(seed, step, stream_id, GCMC_RANDOM_C, attempt)
        theta = math.pi * (2.0 * uniform(h[2], h[3]) - 1.0)
        axis = min(int(math.floor(3.0 * uniform(k[0], k[1]))), 2)
        ref = new[int(bead)]
        new = ref + (new - ref) @ rotation_matrix(theta, axis).T
    return new


def in_block_pocket(blocks, i: int, kinds, positions) -> bool:
    """``inblockpocket`` (montecarlo.jl:631-640): some atom in the species block of ``i`` or in the atom block of its kind"""
    return any(blocks.species_blocked(i, p) or blocks.atom_blocked(int(kinds[a]), p) for a, p in enumerate(positions))


def propose_gcmc(seed: int, step: int, stream_id: int, species_of_molecules, positions_of_molecules, species, mat, dmax: float,
                 thetamax: float, max_molecules: int = None, blocks=None) -> GcmcProposal:
    """What stream ``stream_id`` proposes at the absolute step ``step`` of ``ceg_mc_group_sweep_gcmc`` for a chain whose molecule
    ``d`` (device molecule order) is of species ``species_of_molecules[d]`` and sits at ``positions_of_molecules[d]``.
    ``species``: one :class:`GcmcSpecies` per species; ``mat``: the MC cell (columns); ``thetamax`` in radians.

    ``blocks`` (an object with ``species_blocked(i, point)`` and ``atom_blocked(kind, point)``, e.g. :class:`Blocks`; the species need
    their ``kinds``): the block-pocket rules of ``choose_step!`` (simulation.jl:271-326).  Translation, rotation and random_rotation
    are tested once; random_translation and random_reinsertion take the first of 1000 attempts outside every pocket; an insertion takes
    the first attempt whose bead lies outside the species block and is pocket-blocked if the whole placement is not."""
    u = acceptance_draw(seed, step, stream_id)
    ns = len(species)
    w = draw(seed, step, stream_id, GCMC_SELECT)
    i = min(int(math.floor(uniform(w[0], w[1]) * ns)), ns - 1)
    sp = species[i]
    kind = sp.moves(uniform(w[2], w[3]))
    wm = draw(seed, step, stream_id, GCMC_MOLECULE)
    if kind == 5 and uniform(wm[2], wm[3]) < 0.5:
        kind = SWAP_DELETION
    members = [d for d, s in enumerate(species_of_molecules) if s == i]
    n_i, nmol = len(members), len(species_of_molecules)
    none = np.empty((0, 3))
    if kind == SWAP_INSERTION:
        if max_molecules is not None and nmol >= max_molecules:
            return GcmcProposal(i, kind, nmol, n_i, none, u, False, True)
        mol, pos = nmol, np.asarray(sp.model, dtype=np.float64).reshape(-1, 3)
    else:
        if n_i == 0:
            return GcmcProposal(i, kind, -1, 0, none, u, True, False)
        mol = members[min(int(math.floor(uniform(wm[0], wm[1]) * n_i)), n_i - 1)]
        pos = np.asarray(positions_of_molecules[mol], dtype=np.float64).reshape(-1, 3)
        if kind == SWAP_DELETION:
            return GcmcProposal(i, kind, mol, n_i, none, u, False, False)

    def tested(new):          # a kind that is not retried: the one proposal, pocket-blocked or not
        return GcmcProposal(i, kind, mol, n_i, new, u, False, False, 0, blocks is not None and in_block_pocket(blocks, i, sp.kinds, new))

    if kind in (TRANSLATION, ROTATION):
        if kind == ROTATION and len(pos) == 1:
            return tested(pos.copy())
        g = draw(seed, step, stream_id, GEOMETRY_A)
        if kind == TRANSLATION:
            h = draw(seed, step, stream_id, GEOMETRY_B)
            r = np.array([(2.0 * uniform(g[0], g[1]) - 1.0) * dmax, (2.0 * uniform(g[2], g[3]) - 1.0) * dmax,
                          (2.0 * uniform(h[0], h[1]) - 1.0) * dmax])
            return tested(pos + r)
        theta = thetamax * (2.0 * uniform(g[0], g[1]) - 1.0)
        axis = min(int(math.floor(3.0 * uniform(g[2], g[3]))), 2)
        ref = pos[int(sp.bead)]
        return tested(ref + (pos - ref) @ rotation_matrix(theta, axis).T)

    if blocks is None or kind == RANDOM_ROTATION:
        return tested(random_placement(seed, step, stream_id, kind, pos, sp.bead, mat))
    for attempt in range(ATTEMPTS):
        new = random_placement(seed, step, stream_id, kind, pos, sp.bead, mat, attempt)
        if kind == SWAP_INSERTION:
            if not blocks.species_blocked(i, new[int(sp.bead)]):
                return GcmcProposal(i, kind, mol, n_i, new, u, False, False, attempt, in_block_pocket(blocks, i, sp.kinds, new))
        elif not in_block_pocket(blocks, i, sp.kinds, new):
            return GcmcProposal(i, kind, mol, n_i, new, u, False, False, attempt, False)
    return GcmcProposal(i, kind, mol, n_i, none, u, False, False, ATTEMPTS - 1, True)


def tail_change(tail_framework: float, tail_cross_row, counts, i: int, num: int) -> float:
    """``modify_species_dryrun(tc, i, num)`` (tailcorrection.jl:86-96) in the order the device evaluates it"""
    d = float(tail_framework)
    for j, nj in enumerate(counts):
        d += (float(num) + 2.0 * float(nj) if j == i else 2.0 * float(nj)) * float(tail_cross_row[j])
    return d * float(num)


def swap_threshold(row, temperature: float, n_species: int, phiPV_div_k: float, self_reciprocal: float, tc: float, insertion: bool):
    """(diff, threshold) of ``compute_accept_move`` / ``compute_accept_move_swap`` (montecarlo.jl:705-707, gcmc.jl:77-88) for a swap:
    ``row`` = the insertion row, or ``movement_energy`` of the molecule to delete; the move is accepted iff ``u < threshold``."""
    E = ((float(row[0]) + float(row[1])) + float(row[2])) + float(row[3])
    with np.errstate(over="ignore", under="ignore"):
        if insertion:
            diff = (E - self_reciprocal) + tc
            thr = ((phiPV_div_k / temperature) / float(n_species + 1)) * float(np.exp(np.float64(-diff / temperature)))
        else:
            diff = -(E - self_reciprocal) + tc
            thr = ((float(n_species) * temperature) / phiPV_div_k) * float(np.exp(np.float64(-diff / temperature)))
    return diff, thr


def swap_rule(row, u: float, temperature: float, n_species: int, phiPV_div_k: float, self_reciprocal: float, tc: float,
              insertion: bool) -> bool:
    """The swap decision of ``ceg_mc_group_sweep_gcmc``; a blocked insertion (framework vdw >= 1e90) is rejected."""
    if insertion and row[0] >= 1e90:
        return False
    return bool(u < swap_threshold(row, temperature, n_species, phiPV_div_k, self_reciprocal, tc, insertion)[1])


# ---- the sampler of a chain group (``ceg_mc_group_set_sampler``): the bin of a position as bin_trajectory computes it
# (averageclusters.jl:154-202), the frames of a sweep, and the positions of a chain followed through a sweep's log
def bin_index(unit_invmat, dims, p) -> np.ndarray:
    """0-based bin (i_a, i_b, i_c) of the position(s) ``p[..., 3]`` on a map of ``dims = (na, nb, nc)`` bins over the unit cell
    whose inverse matrix is ``unit_invmat`` (3x3, ``y = unit_invmat @ p``), in the device's operation order:
    ``y_r = (I[r,0] p_x + I[r,1] p_y) + I[r,2] p_z``, ``u = y - floor(y)``, ``i = ceil(u n) + (u == 0) - 1`` (:182-184), clamped to
    ``[0, n - 1]``."""
    return bin_index_fractional(fractional(unit_invmat, p), dims)


def fractional(unit_invmat, p) -> np.ndarray:
    """``y[..., 3]`` of :func:`bin_index`: the unfloored fractional coordinates, each a sum of three products left to right"""
    I = np.asarray(unit_invmat, dtype=np.float64).reshape(3, 3)
    p = np.asarray(p, dtype=np.float64)
    return np.stack([(I[r, 0] * p[..., 0] + I[r, 1] * p[..., 1]) + I[r, 2] * p[..., 2] for r in range(3)], axis=-1)


def bin_index_fractional(y, dims) -> np.ndarray:
    y = np.asarray(y, dtype=np.float64)
    n = np.asarray(dims, dtype=np.int64).reshape(3)
    u = y - np.floor(y)
    i = np.ceil(u * n.astype(np.float64)).astype(np.int64) + (u == 0.0) - 1
    return np.clip(i, 0, n - 1)


def bin_positions(bins, unit_invmat, positions, symmetries=()) -> np.ndarray:
    """Add the positions ``[n, 3]`` to ``bins[nc, nb, na]`` (one (map, channel) block of the sampler: ``a`` fastest), each once as it
    is and once per symmetry operation ``(R[3, 3], t[3])`` -- or row block ``[3, 4] = (R | t)`` -- applied to the unfloored
    fractional coordinates: ``y'_r = ((R[r,0] y_0 + R[r,1] y_1) + R[r,2] y_2) + t_r`` (:185-188).  -> ``bins``."""
    nc, nb, na = bins.shape
    y = fractional(unit_invmat, np.asarray(positions, dtype=np.float64).reshape(-1, 3))
    images = [y]
    for op in symmetries:
        S = np.concatenate([np.asarray(op[0], dtype=np.float64).reshape(3, 3), np.asarray(op[1], dtype=np.float64).reshape(3, 1)], axis=1) \
            if len(op) == 2 else np.asarray(op, dtype=np.float64).reshape(3, 4)
        images.append(np.stack([((S[r, 0] * y[:, 0] + S[r, 1] * y[:, 1]) + S[r, 2] * y[:, 2]) + S[r, 3] for r in range(3)], axis=-1))
    for img in images:
        i = bin_index_fractional(img, (na, nb, nc))
        np.add.at(bins, (i[:, 2], i[:, 1], i[:, 0]), 1)
    return bins


def sampler_frames(first_step: int, nsteps: int, every: int, from_step: int = 0) -> list:
    """The absolute steps after which a sweep of ``nsteps`` steps from ``first_step`` takes a frame: ``s >= from_step`` and
    ``(s + 1) % every == 0``, in step order."""
    if every < 1 or from_step < 0:
        raise ValueError("every >= 1 and from_step >= 0")
    lo = max(int(first_step), int(from_step))
    s = lo + (-(lo + 1)) % every                   # the first s >= lo with (s + 1) % every == 0
    return list(range(s, int(first_step) + max(int(nsteps), 0), every))


# The recorder of ``ceg_mc_group_set_recorder`` (csrc/ceg_mc_record.hip): when a frame is due and how the minimum is followed.
def snapshot_due(cc: int, origin: int, every: int) -> bool:
    """A frame at the end of cycle ``cc``: ``every > 0 and cc >= origin and (cc - origin) % every == 0``."""
    if every < 0 or origin < 0:
        raise ValueError("every >= 0 and origin >= 0")
    return every > 0 and cc >= origin and (cc - origin) % every == 0


def snapshot_cycles(cycle0: int, ncycles: int, origin: int, every: int) -> list:
    """The cycles ``cc`` of a call (``cycle0 <= cc < cycle0 + ncycles``) at whose end a frame is due, in order."""
    return [cc for cc in range(int(cycle0), int(cycle0) + max(int(ncycles), 0)) if snapshot_due(cc, origin, every)]


def track_minimum(energies, e0, stopped=None, cycle0: int = 1):
    """``RMinimumEnergy`` per chain over ``energies`` [ncycles, K] (row j: the end of cycle ``cycle0 + j``) from the initial
    minimum ``e0`` [K] (``mink`` = -1): ``if e < mine`` -- strict, so a tie keeps the earlier cycle, and a NaN never wins.
    ``stopped`` [ncycles, K] bool: the chain is not tested at that cycle end.  -> (mink int64[K], mine float64[K])."""
    E = np.asarray(energies, dtype=np.float64)
    mine = np.array(e0, dtype=np.float64, copy=True).reshape(-1)
    E = E.reshape(-1, len(mine))
    mink = np.full(len(mine), -1, dtype=np.int64)
    S = np.zeros(E.shape, dtype=bool) if stopped is None else np.asarray(stopped, dtype=bool).reshape(E.shape)
    for j in range(E.shape[0]):
        for c in range(E.shape[1]):
            if not S[j, c] and E[j, c] < mine[c]:
                mine[c], mink[c] = E[j, c], int(cycle0) + j
    return mink, mine


def replay_positions(start_positions, records, atoms_per_species=None, start_species=None):
    """Follow one chain through the log of a sweep (``records``: the chain's column of the log of ``sweep`` or ``sweep_gcmc``) from
    ``start_positions`` (one ``[m, 3]`` array per molecule, device molecule order): an accepted displacement replaces the molecule's
    atoms by the logged placement, an accepted insertion appends ``atoms_per_species[species]`` atoms as the last molecule, an
    accepted deletion moves the last molecule into the hole.  Yields, after every step, the list of the molecules' positions --
    with ``start_species`` (the species of every molecule) pairs ``(species, positions)``."""
    mols = [np.array(p, dtype=np.float64).reshape(-1, 3) for p in start_positions]
    spec = None if start_species is None else [int(s) for s in start_species]
    gcmc = "species" in (records.dtype.names or ())
    for rec in records:
        kind, d = int(rec["kind"]), int(rec["molecule"])
        if rec["accepted"]:
            if gcmc and kind == SWAP_INSERTION:
                mols.append(np.array(rec["positions"][:int(atoms_per_species[int(rec["species"])])], dtype=np.float64))
                if spec is not None:
                    spec.append(int(rec["species"]))
            elif gcmc and kind == SWAP_DELETION:
                mols[d] = mols[-1]
                mols.pop()
                if spec is not None:
                    spec[d] = spec[-1]
                    spec.pop()
            else:
                mols[d] = np.array(rec["positions"][:len(mols[d])], dtype=np.float64)
        yield list(mols) if spec is None else (list(spec), list(mols))


# ---- neighbour cells (``ceg_mc_group_set_device_cells``): the cell lists of a chain, i.e. ``CellMirror`` of csrc/ceg_mc_state.h, whose
# sequential semantics the accept launch of csrc/ceg_mc_cells.hip replays.  The order of the entries of a cell fixes the order of the
# pair sum of every later row, so the three operations are restated exactly.
class CellBook:
    """Which atom slot sits at which entry of which cell.  ``invmat``: the inverse of the MC cell matrix (``mc.invmat``, fractional =
    invmat @ p); ``nb``: bins per axis (:meth:`ceg_hip.energy.DeviceMonteCarlo.neighbour_cells`).  ``members[c]`` lists the atom slots
    of cell ``c`` in entry order; ``cell_of`` / ``idx_of`` map an atom slot to its cell and entry (absent: in no cell); ``max_fill``
    is the longest list there has been (the capacity a handle needs)."""

    def __init__(self, invmat, nb):
        self.invmat = np.asarray(invmat, dtype=np.float64).reshape(3, 3)
        self.nb = tuple(int(n) for n in nb)
        self.members = [[] for _ in range(self.nb[0] * self.nb[1] * self.nb[2])]
        self.cell_of, self.idx_of = {}, {}
        self.max_fill = 0

    def bin_of(self, p) -> int:
        """``cell_of_position`` (csrc/ceg_consumers.h): f = invmat p in that order of operations, f - floor(f), the truncation of
        ``f * nb`` and both clamps (f - floor(f) rounds to 1.0 for a tiny negative f: the upper clamp)."""
        x, y, z = (float(v) for v in p)
        b = []
        for i in range(3):
            I = self.invmat[i]
            f = (float(I[0]) * x + float(I[1]) * y) + float(I[2]) * z
            f -= math.floor(f)
            q = int(f * self.nb[i])
            b.append(0 if q < 0 else (self.nb[i] - 1 if q >= self.nb[i] else q))
        return (b[0] * self.nb[1] + b[1]) * self.nb[2] + b[2]

    def take_out(self, slot: int) -> None:
        """the last entry of the cell moves into the hole, and its ``idx_of`` follows"""
        slot = int(slot)
        if slot not in self.cell_of:
            return
        c, i = self.cell_of.pop(slot), self.idx_of.pop(slot)
        mem = self.members[c]
        moved = mem[-1]
        mem[i] = moved
        if moved != slot:
            self.idx_of[moved] = i
        mem.pop()

    def put_in(self, slot: int, c: int) -> None:
        """append"""
        mem = self.members[int(c)]
        mem.append(int(slot))
        self.cell_of[int(slot)], self.idx_of[int(slot)] = int(c), len(mem) - 1
        self.max_fill = max(self.max_fill, len(mem))

    def refresh(self, slot: int) -> None:
        """the record of the atom is copied again where it sits: the lists do not change"""

    def set_atoms(self, positions) -> "CellBook":
        """``ceg_mc_set_guests``: every atom slot put in, in slot order"""
        for slot, p in enumerate(np.asarray(positions, dtype=np.float64).reshape(-1, 3)):
            self.put_in(slot, self.bin_of(p))
        return self

    def move(self, first: int, positions) -> int:
        """an accepted displacement of the molecule in atom slots ``first ...`` (``accept_cell_ops``), per atom in order: refresh where
        the bin did not change, else take-out and put-in -> the number of atoms that changed their cell"""
        changed = 0
        for a, p in enumerate(np.asarray(positions, dtype=np.float64).reshape(-1, 3)):
            c = self.bin_of(p)
            if self.cell_of.get(first + a) == c:
                self.refresh(first + a)
                continue
            self.take_out(first + a)
            self.put_in(first + a, c)
            changed += 1
        return changed

    def insert(self, first: int, positions) -> None:
        """an accepted insertion into the atom slots ``first ...``: put-in of the atoms in order"""
        for a, p in enumerate(np.asarray(positions, dtype=np.float64).reshape(-1, 3)):
            self.put_in(first + a, self.bin_of(p))

    def remove(self, first: int, m: int, last_first: int = -1, last_m: int = 0) -> None:
        """an accepted deletion of the molecule in atom slots ``first ... first + m - 1``: take-out of its atoms in order, then the
        refresh of the atoms of the last molecule (slots ``last_first ...``) where that one takes over the index"""
        for a in range(m):
            self.take_out(first + a)
        for a in range(last_m):
            self.refresh(last_first + a)

    def lists(self, nslots: int):
        """-> (int32[nslots] cell, int32[nslots] entry), -1 where the slot is in no cell: what ``DeviceMonteCarlo.cell_lists`` returns"""
        cell_of, idx_of = np.full(int(nslots), -1, dtype=np.int32), np.full(int(nslots), -1, dtype=np.int32)
        for slot, c in self.cell_of.items():
            cell_of[slot], idx_of[slot] = c, self.idx_of[slot]
        return cell_of, idx_of


def replay_cell_book(book: CellBook, records, first_slot, atoms) -> int:
    """Follow one chain's cell lists through the log of a plain sweep (``records``: the chain's column of the log of ``sweep``):
    every accepted displacement of device molecule ``d`` moves the atoms in slots ``first_slot[d] ... + atoms[d] - 1`` to the logged
    placement.  Idle and stopped steps (molecule < 0) change nothing.  -> the number of atoms that changed their cell."""
    changed = 0
    for rec in records:
        d = int(rec["molecule"])
        if d >= 0 and rec["accepted"]:
            changed += book.move(int(first_slot[d]), rec["positions"][:int(atoms[d])])
    return changed


# ---- cycles (``ceg_mc_group_sweep_cycles`` / ``ceg_mc_group_sweep_gcmc_cycles``): the end-of-cycle block of run_montecarlo!
# (simulation.jl:818-827) in the operation order of ``k_mcg_cycle_end``, thetamax in radians as the ABI holds it
ADAPT_DMAX, ADAPT_THETAMAX = 1, 2
DMAX_MIN, DMAX_MAX = 0.1, 3.0
THETAMAX_MIN, THETAMAX_MAX, THETAMAX_GAIN = 0.17453292519943295, 3.141592653589793, 2.0943951023931953      # 10, 180 and 120 degrees


def _clamp(x: float, lo: float, hi: float) -> float:
    return hi if x > hi else (lo if x < lo else x)


def adapt_dmax(dmax: float, accepted: int, trials: int, cc: int) -> float:
    """``statistics.dmax`` after cycle ``cc`` (the reference's ``counter_cycle``, >= 1) from the cumulative translation counters
    (simulation.jl:818-822); unchanged with zero trials (the reference's NaN ratio)."""
    if trials <= 0:
        return float(dmax)
    r = float(accepted) / float(trials)
    q = 10.0 / float(99 + cc)
    s = math.sqrt(q)
    f = (r - 0.25) * s
    g = 1.0 + f
    return _clamp(float(dmax) * g, DMAX_MIN, DMAX_MAX)


def adapt_thetamax(thetamax: float, accepted: int, trials: int, cc: int) -> float:
    """``statistics.θmax`` in radians after cycle ``cc`` from the cumulative rotation counters (simulation.jl:823-826); unchanged with
    zero trials.  A restatement in radians: not bit-equal to the reference's arithmetic in degrees."""
    if trials <= 0:
        return float(thetamax)
    r = float(accepted) / float(trials)
    a = (r - 0.5) / float(cc)
    b = a * THETAMAX_GAIN
    return _clamp(float(thetamax) + b, THETAMAX_MIN, THETAMAX_MAX)


def cycle_records(temperatures, dmax: float, thetamax: float, counters, nmol, delta_moves=None, delta_swaps=None, *, cycle0: int = 1,
                  adapt: int = ADAPT_DMAX | ADAPT_THETAMAX, prior=(0, 0, 0, 0)) -> np.ndarray:
    """The records (``_abi.MC_CYCLE_RECORD_DTYPE`` [ncycles]) ``k_mcg_cycle_end`` writes for ONE chain that starts the call with
    ``dmax`` / ``thetamax``: ``temperatures[j]`` in force during cycle ``j``, ``counters[j]`` = the CALL's (translation trials, accepted,
    rotation trials, accepted) as they stand at the end of cycle ``j`` (``prior`` is added), ``nmol[j]`` the chain's molecules then,
    ``delta_moves[j]`` / ``delta_swaps[j]`` the call's sums then (None: zeros).  A chain without molecules at a cycle end, a kind with
    zero trials and a clear ``adapt`` bit carry the value over."""
    from ._abi import MC_CYCLE_RECORD_DTYPE
    n = len(temperatures)
    out = np.zeros(n, dtype=MC_CYCLE_RECORD_DTYPE)
    d, t = float(dmax), float(thetamax)
    for j in range(n):
        tt, ta, rt, ra = (int(p) + int(x) for p, x in zip(prior, counters[j]))
        cc = int(cycle0) + j
        live = int(nmol[j]) > 0
        dn = adapt_dmax(d, ta, tt, cc) if live and adapt & ADAPT_DMAX else d
        tn = adapt_thetamax(t, ra, rt, cc) if live and adapt & ADAPT_THETAMAX else t
        out[j] = (float(temperatures[j]), d, t, dn, tn, 0.0 if delta_moves is None else float(delta_moves[j]),
                  0.0 if delta_swaps is None else float(delta_swaps[j]), tt, ta, rt, ra, int(nmol[j]), 0)
        d, t = dn, tn
    return out


# ------------------------------------------------------------------ tempering (ceg_mc_group_set_tempering)
# The exchange round of ``k_mcg_exchange`` (csrc/ceg_mc_temper.hip) in its operation order: what the device is held to.
EXCHANGE = 9              # the purpose of the exchange draw, on the stream of the pair's chain on the lower rung


def exchange_pairs(k: int, cc: int, every: int) -> list:
    """The rung pairs ``(r, r + 1)`` of the round at the end of cycle ``cc`` (the reference's ``counter_cycle``) of ``k`` chains: none
    unless ``cc % every == 0``; else ``r = parity, parity + 2, ...`` with ``r + 1 < k`` and ``parity = (cc // every) & 1``."""
    if every < 1:
        raise ValueError("every >= 1")
    if int(cc) % int(every) != 0:
        return []
    parity = (int(cc) // int(every)) & 1
    return [(r, r + 1) for r in range(parity, int(k) - 1, 2)]


def exchange_threshold(E_a: float, E_b: float, T_a: float, T_b: float) -> float:
    """``e`` of the rule for the chain ``a`` on the lower and ``b`` on the upper rung (simulation.jl:533), every operation rounded to
    FP64 in this order: ``ia = 1 / T_a; ib = 1 / T_b; d = ia - ib; Tp = 1 / d; x = (E_a - E_b) / Tp; e = exp(x)``.  Equal temperatures
    give ``Tp = inf`` and ``e = 1``; NaN energies give NaN."""
    with np.errstate(all="ignore"):
        ia = np.float64(1.0) / np.float64(T_a)
        ib = np.float64(1.0) / np.float64(T_b)
        d = ia - ib
        Tp = np.float64(1.0) / d
        x = float((np.float64(E_a) - np.float64(E_b)) / Tp)
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def exchange_rule(E_a: float, E_b: float, u: float, threshold: float) -> bool:
    """``E_b < E_a || u < e``: NaN energies reject"""
    return bool(E_b < E_a or u < threshold)


def exchange_round(rung, energy, temperatures_by_rung, stopped, seed: int, step: int, stream_id, cc: int, every: int,
                   next_temperatures_by_rung=None):
    """One cycle end of ``k_mcg_exchange`` for K chains: ``rung[c]`` the rung of chain ``c`` during the ended cycle, ``energy[c]`` its
    energy at the end, ``temperatures_by_rung[r]`` the temperature in force on rung ``r`` during the ended cycle, ``stopped[c]`` whether
    the chain is stopped at ``step``, the cycle's absolute last step; ``cc`` the cycle's counter.  ``next_temperatures_by_rung``: the next
    cycle's (default: the same).  A pair is attempted if the round is due and neither chain is stopped; the draw is
    ``U(w0, w1)`` of ``draw(seed, step, stream_id[a], EXCHANGE)``.
    -> (the rungs of the next cycle int32[K], records ``_abi.MC_EXCHANGE_RECORD_DTYPE`` [K])"""
    from ._abi import MC_EXCHANGE_RECORD_DTYPE
    k = len(rung)
    rung = [int(r) for r in rung]
    if sorted(rung) != list(range(k)):
        raise ValueError("rung: a permutation of 0..K-1")
    T = [float(t) for t in temperatures_by_rung]
    Tn = T if next_temperatures_by_rung is None else [float(t) for t in next_temperatures_by_rung]
    chain = [0] * k
    for c, r in enumerate(rung):
        chain[r] = c
    new = list(rung)
    rec = np.zeros(k, dtype=MC_EXCHANGE_RECORD_DTYPE)
    rec["rung"], rec["partner"], rec["accepted"], rec["energy"] = rung, -1, -1, [float(e) for e in energy]
    for r, _ in exchange_pairs(k, cc, every):
        a, b = chain[r], chain[r + 1]
        if stopped[a] or stopped[b]:
            continue
        w = draw(seed, step, int(stream_id[a]), EXCHANGE)
        u = uniform(w[0], w[1])
        e = exchange_threshold(float(energy[a]), float(energy[b]), T[r], T[r + 1])
        acc = exchange_rule(float(energy[a]), float(energy[b]), u, e)
        for me, other in ((a, b), (b, a)):
            rec[me]["partner"], rec[me]["accepted"], rec[me]["u"], rec[me]["threshold"] = other, int(acc), u, e
        if acc:
            new[a], new[b] = r + 1, r
    rec["rung_next"] = new
    rec["temperature_next"] = [Tn[r] for r in new]
    return np.array(new, dtype=np.int32), rec


# ------------------------------------------------------------------ isotherms (ceg_mc_group_set_chain_plan)
def isotherm_ncycles(ncycles: int, pressure_pa: float) -> int:
    """The run length ``make_isotherm`` gives the chain of one pressure (parameterinputs.jl:319):
    ``ceil(Int, simu.ncycles * (1 + 1e3 / ustrip(u"Pa", P)))``"""
    return int(math.ceil(int(ncycles) * (1 + 1e3 / float(pressure_pa))))


def accessible_volume(mask, unitcell, supercell) -> float:
    """``GCMCData.volumes[i]`` in A^3 (gcmc.jl:26-37): ``accessible_fraction * (det(unitcell) * Π)`` with ``Π`` the product of
    ``supercell`` and ``accessible_fraction = 1 - count(block) / length(block)`` of the species' block mask (``None`` or an empty mask:
    1).  ``unitcell``: the cell vectors as columns."""
    M = np.asarray(unitcell, dtype=np.float64).reshape(3, 3)
    det = (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
           + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))
    pi = 1
    for x in (supercell if np.ndim(supercell) else (supercell,)):
        pi *= int(x)
    cellvolume = float(det) * pi
    fraction = 1.0
    if mask is not None and np.size(mask) > 0:
        fraction = 1.0 - int(np.count_nonzero(mask)) / int(np.size(mask))
    return fraction * cellvolume


def phiPV_div_k(phi: float, pressure_pa: float, volume_A3: float) -> float:
    """``φPV_div_k`` of one species in K (simulation.jl:714-715): ``φ * uconvert(u"K", abs(P) * V / u"k")`` with P in Pa, V in A^3
    (1e-30 m^3) and k = 1.380649e-23 J/K.  The fugacity coefficient ``phi`` is the caller's (Clapeyron's in the reference, :707-712)."""
    return float(phi) * (abs(float(pressure_pa)) * float(volume_A3) * 1e-30 / 1.380649e-23)


# ------------------------------------------------------------------ site hopping (ceg_site_group_*, csrc/ceg_site.hip)
# The reference's second Monte-Carlo model (src/sitehopping.jl): m molecules on n sites, all physics in ``frameworkenergies[n]`` and
# ``interactions[n, n]`` (symmetric, the diagonal 1e100).  Sites are 0-based here, as on the device.  The step of stream ``c`` at the
# absolute step ``s``:
#   10 SITE_SELECT  molecule ``i = min(floor(U(w0, w1) m), m - 1)``, site ``new = min(floor(U(w2, w3) n), n - 1)``
#   3  acceptance   ``u = U(w0, w1)``
#   before = framework[old] + R(old), after = framework[new] + R(new), R the row sum in the device's order (:func:`site_row_sum`);
#   accepted iff ``after < before`` or ``u < exp((before - after) / T)``; then ``energy += after - before`` and ``population[i] = new``.
# A hop onto an occupied site meets 1e100 and is rejected by the rule; a hop onto the own site has after == before and is accepted.
#   11 SITE_POPULATE  :func:`site_random_population`, the host-side start of ``run_random_quenching``; never drawn on the device.
SITE_SELECT = 10
SITE_POPULATE = 11
_LANES = np.arange(64)


def site_propose(seed: int, step: int, stream_id: int, m: int, n: int):
    """-> (molecule ``i``, site ``new``, acceptance draw ``u``) of stream ``stream_id`` at the absolute step ``step``."""
    w = draw(seed, step, stream_id, SITE_SELECT)
    i = min(int(math.floor(uniform(w[0], w[1]) * float(m))), m - 1)
    new = min(int(math.floor(uniform(w[2], w[3]) * float(n))), n - 1)
    return i, new, acceptance_draw(seed, step, stream_id)


def site_row_sum(terms) -> float:
    """The sum of ``terms`` [m] in the order of ``k_site_sweep``, a fixed function of m alone: lane ``l`` of 64 adds its terms
    ``l, l + 64, l + 128, ...`` in rising order onto +0.0; then for ``o = 32, 16, 8, 4, 2, 1`` every lane replaces its sum by
    (its sum) + (the sum of lane ``l ^ o``); the result is lane 0's.  The caller puts +0.0 where a term is left out (the same bits:
    such a sum is never -0.0)."""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    rows = -(-len(t) // 64)
    padded = np.zeros(rows * 64, dtype=np.float64)
    padded[:len(t)] = t
    lanes = np.zeros(64, dtype=np.float64)
    for r in padded.reshape(rows, 64):          # (+0.0 for the lanes whose terms have run out: bit-neutral)
        lanes = lanes + r
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[_LANES ^ o]
    return float(lanes[0])


def site_movement_energy(framework, interactions, population, i: int, site=None) -> float:
    """``movement_energy(sh, i, si)`` (sitehopping.jl:114-121) in the device's order: ``framework[site] + R(site)`` with
    ``R = site_row_sum(interactions[site, population[j]] for j != i, +0.0 at j == i)``.  ``site=None``: where molecule ``i`` sits."""
    pop = np.asarray(population, dtype=np.int64)
    s = int(pop[i]) if site is None else int(site)
    terms = np.array(np.asarray(interactions, dtype=np.float64)[s, pop], dtype=np.float64)
    terms[i] = 0.0
    return float(np.float64(framework[s]) + np.float64(site_row_sum(terms)))


class SiteStep(NamedTuple):
    molecule: int
    old_site: int
    new_site: int
    before: float
    after: float
    u: float
    threshold: float          # exp((before - after) / T), what u is compared with when after >= before
    accepted: bool


def site_step(framework, interactions, population, seed: int, step: int, stream_id: int, temperature: float, decision=None) -> SiteStep:
    """One step of one chain; ``population`` (a mutable integer array) is updated in place when the step is accepted.
    ``decision`` not None: that decision is followed instead of the rule's (a replay of a log across an exp that rounds
    differently on the host).  The caller adds ``after - before`` to its running energy when the step is accepted."""
    m, n = len(population), len(framework)
    i, new, u = site_propose(seed, step, stream_id, m, n)
    old = int(population[i])
    before = site_movement_energy(framework, interactions, population, i, old)
    after = site_movement_energy(framework, interactions, population, i, new)
    with np.errstate(over="ignore"):
        x = float((np.float64(before) - np.float64(after)) / np.float64(temperature))
    try:
        e = math.exp(x)
    except OverflowError:
        e = math.inf
    ok = bool(after < before or u < e)
    if decision is not None:
        ok = bool(decision)
    if ok:
        population[i] = new
    return SiteStep(i, old, new, before, after, u, e, ok)


class SiteReplay(NamedTuple):
    steps: list               # [ncycles * steps_per_cycle] SiteStep
    population: np.ndarray    # uint16[m] at the end
    energy: float             # the running energy at the end
    delta: float              # the sum of the accepted changes added to ``delta``
    cycle_energy: np.ndarray  # float64[ncycles] at the cycle ends
    cycle_population: np.ndarray   # uint16[ncycles, m] at the cycle ends
    accepted: int


def site_replay(framework, interactions, population, energy: float, seed: int, first_step: int, stream_id: int, temperatures,
                steps_per_cycle: int, log=None, delta: float = 0.0) -> SiteReplay:
    """One chain through ``len(temperatures)`` cycles of ``steps_per_cycle`` steps from the absolute step ``first_step``, as
    ``ceg_site_group_sweep_cycles`` runs it.  ``log`` (the chain's column of the device log, with a field ``accepted``): its
    decisions are followed."""
    fw = np.asarray(framework, dtype=np.float64)
    it = np.asarray(interactions, dtype=np.float64)
    pop = np.array(population, dtype=np.int64)
    e, d, acc = np.float64(energy), np.float64(delta), 0
    steps, ce, cp = [], [], []
    t = 0
    for T in temperatures:
        for _ in range(int(steps_per_cycle)):
            dec = None if log is None else bool(log["accepted"][t])
            st = site_step(fw, it, pop, seed, int(first_step) + t, stream_id, float(T), dec)
            if st.accepted:
                diff = np.float64(st.after) - np.float64(st.before)
                e, d, acc = e + diff, d + diff, acc + 1
            steps.append(st)
            t += 1
        ce.append(float(e))
        cp.append(pop.astype(np.uint16))
    m = len(pop)
    return SiteReplay(steps, pop.astype(np.uint16), float(e), float(d), np.array(ce, dtype=np.float64),
                      np.array(cp, dtype=np.uint16).reshape(len(ce), m), acc)


# ---- tempering of site-hopping ladders (ceg_site_group_set_tempering, k_site_sweep_pt; run_parallel_tempering, simulation.jl:461-634)
# The rule, as include/ceg_hip.h states it:
# Layout.  A group of K chains with tempering installed is L = K / R ladders of R rungs.  Chain ``l*R + r`` is rung r of ladder l.
#   A chain index means a rung from then on.  Temperatures, streams, hop counters, cycle records, frames and the minimum belong to
#   the rung.  Population, running ``energy`` and ``delta`` belong to the configuration and travel with it.  So ``energy - delta``
#   stays the baseline that the configuration started from.
# Temperatures.  The temperature table ``[ncycles][K]`` gives the rung temperatures.  Inside every ladder and every cycle they must
#   be strictly increasing with the rung, because the reference sorts ``Ts``.
# Exchange draw.  At the absolute step ``s``, every ladder takes one Philox block.  The purpose is ``SITE_EXCHANGE = 12``.  The
#   stream is the ladder's (``ladder_stream[l]``, or ``l``).  ``v = U(w0, w1)`` chooses the pair.  ``u = U(w2, w3)`` is the
#   acceptance draw.
# Pair table.  The pair is the first ``j`` in ``0..R-2`` with ``v < pair_cdf[j]``.  If there is none, the step has no exchange.
#   Each entry must be finite, in [0, 1] and non-decreasing.  The reference attempts at most the first element of
#   ``randsubseq(1:(Npt-1), 0.1)`` (:528-529).  That is ``pair_cdf[j] = 1 - q_(j+1)`` with ``q_0 = 1`` and
#   ``q_(i+1) = q_i * (1 - p)``, computed by repeated multiplication (:func:`site_exchange_cdf`).
# Exchange attempt.  A step whose pair is ``j`` attempts the exchange of rungs ``j`` and ``j+1`` (:531-543).  ``E_a`` and ``E_b``
#   are the running energies of the two rungs at the start of the step.  ``Tx = 1.0 / (1.0 / T_j - 1.0 / T_(j+1))``, with IEEE
#   divisions in this order.  The exchange is accepted iff ``E_b < E_a``, or else ``u < exp((E_a - E_b) / Tx)``.
# After the attempt.  ``pt_attempted[l][j]`` goes up by 1.  On acceptance ``pt_accepted[l][j]`` goes up by 1.  On acceptance the
#   populations of the two rungs are exchanged, and their ``energy`` and ``delta`` with them.  The two rungs make no hop at this
#   step.  ``attempted`` does not move.  Rung ``j`` logs ``molecule = -1``, ``old_site = new_site = -1``, ``before = E_a``,
#   ``after = E_b``, ``u``, ``accepted``.  Rung ``j+1`` logs ``molecule = -2`` and the same values.  Every other rung of the ladder
#   makes the ordinary step (:func:`site_step`).  It uses its own stream and the same bits as without tempering.
# Cycle ends.  Cycle records, frames and ``track_min`` work per rung.  They use the population and energy that sit on the rung at
#   that moment.
# Replica map.  ``replica[K]`` holds, per rung, the rung (0..R-1) on which the configuration now there sat when tempering was
#   installed.  It is a permutation inside every ladder.
SITE_EXCHANGE = 12


def site_exchange_cdf(rungs: int, p: float = 0.1) -> np.ndarray:
    """The pair table of the reference's schedule, float64[R-1]: the first element of ``randsubseq(1:(R-1), p)`` is pair ``j`` with
    probability ``p (1 - p)^j``, so ``cdf[j] = 1 - q_(j+1)`` with ``q_0 = 1`` and ``q_(i+1) = q_i * (1 - p)`` by repeated
    multiplication in FP64."""
    rungs, p = int(rungs), float(p)
    if rungs < 2 or not 0.0 <= p <= 1.0:
        raise ValueError("rungs >= 2 and p in [0, 1]")
    out, q = np.empty(rungs - 1, dtype=np.float64), np.float64(1.0)
    for j in range(rungs - 1):
        q = q * (np.float64(1.0) - np.float64(p))
        out[j] = np.float64(1.0) - q
    return out


def site_exchange_draw(seed: int, step: int, ladder_stream: int, cdf):
    """-> (pair ``j`` or -1, ``u``) of the ladder at the absolute step ``step``: the first ``j`` with ``U(w0, w1) < cdf[j]``;
    ``u = U(w2, w3)``."""
    w = draw(seed, step, ladder_stream, SITE_EXCHANGE)
    v, u = uniform(w[0], w[1]), uniform(w[2], w[3])
    for j, top in enumerate(cdf):
        if v < float(top):
            return j, u
    return -1, u


def site_exchange_threshold(E_a: float, E_b: float, T_a: float, T_b: float) -> float:
    """``exp((E_a - E_b) / Tx)`` with ``Tx = 1.0 / (1.0 / T_a - 1.0 / T_b)`` for rung ``a`` below rung ``b``, every operation rounded
    to FP64 in this order (the arithmetic of :func:`exchange_threshold`)."""
    return exchange_threshold(E_a, E_b, T_a, T_b)


class SiteLadderReplay(NamedTuple):
    steps: list               # [R] lists of SiteStep per rung; an exchange record has molecule -1 (lower rung) or -2, before = E_a, after = E_b
    population: np.ndarray    # uint16[R, m] by rung at the end
    energy: np.ndarray        # float64[R] by rung at the end
    delta: np.ndarray         # float64[R]
    cycle_energy: np.ndarray  # float64[ncycles, R] at the cycle ends, by rung
    cycle_population: np.ndarray   # uint16[ncycles, R, m]
    attempted: np.ndarray     # int64[R] hops attempted by the rung
    accepted: np.ndarray      # int64[R] hops accepted
    pt_attempted: np.ndarray  # int64[R-1] per pair
    pt_accepted: np.ndarray   # int64[R-1]
    replica: np.ndarray       # int32[R]


def site_ladder_replay(framework, interactions, populations, energies, seed: int, first_step: int, stream_ids, ladder_stream: int,
                       temperatures, steps_per_cycle: int, cdf, log=None, deltas=None, replica=None) -> SiteLadderReplay:
    """One ladder of R rungs through ``len(temperatures)`` cycles as ``k_site_sweep_pt`` runs it.  ``populations`` [R, m],
    ``energies`` [R], ``stream_ids`` [R], ``temperatures`` [ncycles, R] (rising with the rung).  ``log`` [steps, R] (the ladder's
    columns of the device log, with a field ``accepted``): its decisions are followed, for hops and exchanges."""
    fw = np.asarray(framework, dtype=np.float64)
    it = np.asarray(interactions, dtype=np.float64)
    pops = [np.array(p, dtype=np.int64) for p in populations]
    R, m = len(pops), len(pops[0])
    T = np.asarray(temperatures, dtype=np.float64).reshape(-1, R)
    e = [np.float64(x) for x in energies]
    d = [np.float64(0.0)] * R if deltas is None else [np.float64(x) for x in deltas]
    rep = list(range(R)) if replica is None else [int(x) for x in replica]
    att, acc = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    pa, pc = np.zeros(R - 1, dtype=np.int64), np.zeros(R - 1, dtype=np.int64)
    steps, ce, cp = [[] for _ in range(R)], [], []
    t = 0
    for Tc in T:
        for _ in range(int(steps_per_cycle)):
            s = int(first_step) + t
            pair, u = site_exchange_draw(seed, s, ladder_stream, cdf)
            for r in range(R):
                if pair >= 0 and r in (pair, pair + 1):
                    continue
                dec = None if log is None else bool(log["accepted"][t, r])
                st = site_step(fw, it, pops[r], seed, s, int(stream_ids[r]), float(Tc[r]), dec)
                att[r] += 1
                if st.accepted:
                    diff = np.float64(st.after) - np.float64(st.before)
                    e[r], d[r] = e[r] + diff, d[r] + diff
                    acc[r] += 1
                steps[r].append(st)
            if pair >= 0:
                a, b = pair, pair + 1
                E_a, E_b = float(e[a]), float(e[b])
                thr = site_exchange_threshold(E_a, E_b, float(Tc[a]), float(Tc[b]))
                ok = bool(E_b < E_a or u < thr)
                if log is not None:
                    ok = bool(log["accepted"][t, a])
                pa[a] += 1
                if ok:
                    pc[a] += 1
                    pops[a], pops[b] = pops[b], pops[a]
                    e[a], e[b], d[a], d[b] = e[b], e[a], d[b], d[a]
                    rep[a], rep[b] = rep[b], rep[a]
                steps[a].append(SiteStep(-1, -1, -1, E_a, E_b, u, thr, ok))
                steps[b].append(SiteStep(-2, -1, -1, E_a, E_b, u, thr, ok))
            t += 1
        ce.append([float(x) for x in e])
        cp.append([p.astype(np.uint16) for p in pops])
    return SiteLadderReplay(steps, np.array([p.astype(np.uint16) for p in pops], dtype=np.uint16).reshape(R, m), np.array(e, dtype=np.float64),
                            np.array(d, dtype=np.float64), np.array(ce, dtype=np.float64).reshape(len(ce), R),
                            np.array(cp, dtype=np.uint16).reshape(len(cp), R, m), att, acc, pa, pc, np.array(rep, dtype=np.int32))


def site_baseline(framework, interactions, population, tailcorrection: float = 0.0):
    """``baseline_energy(::SiteHopping)`` (sitehopping.jl:105-112) in extended precision:
    tail correction + sum of ``framework[population]`` + sum over i < j of ``interactions[population[i], population[j]]``."""
    pop = np.asarray(population, dtype=np.int64)
    sub = np.asarray(interactions, dtype=np.longdouble)[np.ix_(pop, pop)]
    inter = np.triu(sub, 1).sum(dtype=np.longdouble)
    return np.longdouble(tailcorrection) + np.asarray(framework, dtype=np.longdouble)[pop].sum(dtype=np.longdouble) + inter


def site_random_population(seed: int, stream_id: int, n: int, m: int) -> np.ndarray:
    """A ``randperm``-style start (sitehopping.jl:87-88: ``resize!(randperm(n), m)``): the first ``m`` entries of a Fisher-Yates
    shuffle of ``0..n-1`` driven by purpose 11 of stream ``stream_id``: for ``j = 0..m-1`` the block of step ``j`` gives
    ``r = j + min(floor(U(w0, w1) (n - j)), n - j - 1)`` and entries ``j`` and ``r`` are exchanged.  Duplicate-free by construction."""
    if not 0 <= m <= n <= 65535:
        raise ValueError("0 <= m <= n <= 65535")
    perm = list(range(n))
    for j in range(m):
        w = draw(seed, j, stream_id, SITE_POPULATE)
        r = j + min(int(math.floor(uniform(w[0], w[1]) * float(n - j))), n - j - 1)
        perm[j], perm[r] = perm[r], perm[j]
    return np.array(perm[:m], dtype=np.uint16)


# ---- grouped cycles (ceg_site_group_sweep_grouped, k_site_sweep_grouped; run_montecarlo!(::SiteHopping; groupcycles, restartgroupcycle),
# simulation.jl:917-939, 941, 970-982).  The rule, as include/ceg_hip.h states it:
# A grouped cycle of chain c runs on stream ``stream_id[c]`` at temperature T.  Its absolute steps are s0 .. s0 + spc - 1, where
#   ``spc = steps_per_cycle`` (G m for the reference's ``groupcycles = G``).
# 1. Save.  (P0, E0, D0) is the population, running ``energy`` and ``delta`` at the start of the cycle.
# 2. Restart (only when asked for).  The population becomes the first m entries of a Fisher-Yates shuffle of 0..n-1.  Entry
#    j = 0..m-1 takes the Philox block of (seed, step s0, stream, counter word 3 = ``14 | (j << 8)``), purpose ``SITE_RESTART = 14``.
#    ``r = j + min(floor(U(w0, w1) (n - j)), n - j - 1)``, and entries j and r are exchanged (:func:`site_restart_population`).
#    Then ``energy = baseline_energy`` of that population in the wave's order (:func:`site_baseline_wave`).  Call it Er.  Without a
#    restart, Er = E0.
# 3. Hops.  spc ordinary steps follow, :func:`site_step` bit for bit.  ``energy`` moves with every accepted hop.  The group's
#    ``attempted`` / ``accepted`` counters do not move.  The hops accepted inside the cycle are counted separately.
# 4. Decision.  The block of (seed, s0 + spc - 1, stream, purpose ``SITE_GROUP = 13``) gives ``u = U(w0, w1)``.  With E1 the energy
#    after the hops, the cycle is accepted iff ``E1 < E0``, or else ``u < exp((E0 - E1) / T)``.  A NaN E1 is rejected by the rule
#    itself.  ``attempted += 1``.  Accepted: ``accepted += 1`` and ``delta = D0 + (E1 - E0)``.  Rejected: population, ``energy`` and
#    ``delta`` become P0, E0, D0 again.
# 5. Cycle end.  As without groups, on the state after the decision.
SITE_GROUP = 13
SITE_RESTART = 14


def site_restart_draws(seed: int, step: int, stream_id: int, n: int, m: int) -> list:
    """``r_j`` for j = 0..m-1 of a restart at the absolute step ``step``: the block of counter word 3 = ``14 | (j << 8)`` gives
    ``r_j = j + min(floor(U(w0, w1) (n - j)), n - j - 1)``."""
    if not 0 <= m <= n <= 65535:
        raise ValueError("0 <= m <= n <= 65535")
    out = []
    for j in range(m):
        w = draw(seed, step, stream_id, SITE_RESTART | (j << 8))
        out.append(j + min(int(math.floor(uniform(w[0], w[1]) * float(n - j))), n - j - 1))
    return out


def site_restart_population(seed: int, step: int, stream_id: int, n: int, m: int) -> np.ndarray:
    """The population a restart at the absolute step ``step`` puts in place: the first ``m`` entries of the Fisher-Yates shuffle of
    ``0..n-1`` that exchanges entries j and ``r_j`` (:func:`site_restart_draws`) for j rising.  Found as the device finds it, without
    the n entries: entry j ends as the value that position ``r_j`` held just before exchange j.  That value is the position itself
    unless an earlier exchange q < j had ``r_q`` equal to it; the latest such q put there what position q held just before exchange
    q, and so on down."""
    r = site_restart_draws(seed, step, stream_id, n, m)
    out = np.empty(m, dtype=np.uint16)
    for j in range(m):
        p, top = r[j], j
        while True:
            q = top - 1
            while q >= 0 and r[q] != p:
                q -= 1
            if q < 0:
                break
            p = top = q
        out[j] = p
    return out


def site_baseline_wave(framework, interactions, population, tailcorrection: float = 0.0) -> float:
    """``baseline_energy`` in the order of ``k_site_sweep_grouped``'s restart, a fixed function of m alone.  F: lane ``l`` of 64 adds
    ``framework[pop[j]]`` for ``j = l, l + 64, ...`` in rising order onto +0.0.  E: for the rows ``i = 0 .. m - 2`` in rising order
    lane ``l`` adds ``interactions[pop[i], pop[j]]`` for ``j = i + 1 + l, i + 1 + l + 64, ...`` in rising order onto one accumulator
    per lane that starts at +0.0 and runs through all rows.  F and E each meet by the xor butterfly of :func:`site_row_sum`; the
    result is ``(tailcorrection + F) + E``."""
    pop = np.asarray(population, dtype=np.int64)
    fw = np.asarray(framework, dtype=np.float64)
    it = np.asarray(interactions, dtype=np.float64)
    m = len(pop)
    F = np.float64(site_row_sum(fw[pop]))
    lanes = np.zeros(64, dtype=np.float64)
    for i in range(m - 1):
        t = it[pop[i], pop[i + 1:]]
        rows = -(-len(t) // 64)
        padded = np.zeros(rows * 64, dtype=np.float64)     # (+0.0 where a lane has no term: bit-neutral, a sum from +0.0 is never -0.0)
        padded[:len(t)] = t
        for r in padded.reshape(rows, 64):
            lanes = lanes + r
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[_LANES ^ o]
    return float((np.float64(tailcorrection) + F) + lanes[0])


class SiteGroupedCycle(NamedTuple):
    before: float             # E0
    restart_energy: float     # Er (E0 without a restart)
    after: float              # E1
    u: float
    threshold: float          # exp((E0 - E1) / T), what u is compared with when E1 >= E0
    accepted: bool
    restarted: bool
    hops_accepted: int
    restart_population: Optional[np.ndarray]      # uint16[m] what the restart put in place, or None


class SiteGroupedReplay(NamedTuple):
    steps: list               # [ncycles * steps_per_cycle] SiteStep
    cycles: list              # [ncycles] SiteGroupedCycle
    population: np.ndarray    # uint16[m] at the end
    energy: float
    delta: float
    cycle_energy: np.ndarray  # float64[ncycles] at the cycle ends, after the decision
    cycle_delta: np.ndarray   # float64[ncycles]
    cycle_population: np.ndarray   # uint16[ncycles, m]
    attempted: int            # cycles
    accepted: int             # cycles accepted


def site_grouped_replay(framework, interactions, population, energy: float, seed: int, first_step: int, stream_id: int, temperatures,
                        steps_per_cycle: int, restart: bool = False, tailcorrection: float = 0.0, log=None, grouped=None,
                        delta: float = 0.0) -> SiteGroupedReplay:
    """One chain through ``len(temperatures)`` grouped cycles of ``steps_per_cycle`` steps from the absolute step ``first_step``, as
    ``ceg_site_group_sweep_grouped`` runs it.  ``log`` (the chain's column of the device log) and ``grouped`` (its column of the
    grouped records), each with a field ``accepted``: their decisions are followed, for the hops and for the cycles."""
    fw = np.asarray(framework, dtype=np.float64)
    it = np.asarray(interactions, dtype=np.float64)
    pop = np.array(population, dtype=np.int64)
    n, m, spc = len(fw), len(pop), int(steps_per_cycle)
    e, d = np.float64(energy), np.float64(delta)
    att = acc = 0
    steps, cycles, ce, cd, cp = [], [], [], [], []
    t = 0
    for cyc, T in enumerate(temperatures):
        s0 = int(first_step) + t
        P0, E0, D0 = pop.copy(), e, d
        fresh = None
        if restart:
            fresh = site_restart_population(seed, s0, stream_id, n, m)
            pop[:] = fresh
            e = np.float64(site_baseline_wave(fw, it, pop, tailcorrection))
        Er, hops = e, 0
        for _ in range(spc):
            dec = None if log is None else bool(log["accepted"][t])
            st = site_step(fw, it, pop, seed, int(first_step) + t, stream_id, float(T), dec)
            if st.accepted:
                e = e + (np.float64(st.after) - np.float64(st.before))
                hops += 1
            steps.append(st)
            t += 1
        w = draw(seed, s0 + spc - 1, stream_id, SITE_GROUP)
        u, E1 = uniform(w[0], w[1]), e
        with np.errstate(over="ignore", invalid="ignore"):
            x = float((E0 - E1) / np.float64(T))
        try:
            thr = math.exp(x)
        except OverflowError:
            thr = math.inf
        ok = bool(E1 < E0 or u < thr)
        if grouped is not None:
            ok = bool(grouped["accepted"][cyc])
        att += 1
        if ok:
            acc += 1
            d = D0 + (E1 - E0)
        else:
            pop[:] = P0
            e, d = E0, D0
        cycles.append(SiteGroupedCycle(float(E0), float(Er), float(E1), u, thr, ok, bool(restart), hops, fresh))
        ce.append(float(e))
        cd.append(float(d))
        cp.append(pop.astype(np.uint16))
    return SiteGroupedReplay(steps, cycles, pop.astype(np.uint16), float(e), float(d), np.array(ce, dtype=np.float64), np.array(cd, dtype=np.float64),
                             np.array(cp, dtype=np.uint16).reshape(len(ce), m), att, acc)
