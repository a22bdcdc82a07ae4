"""The random stream and the move proposals of the Monte-Carlo sweeps (``ceg_mc_group_sweep``), restated in NumPy.

Needs no device.  The kernels of ``csrc/ceg_mc.hip`` (through ``csrc/ceg_philox.h``) and this module follow the
specification in ``include/ceg_hip.h`` word for word: Philox4x32-10, one block per (step, stream, purpose), nothing random
stored.  A caller uses it to audit a sweep's log, to replay a chain on the host, or to predict what a chain will propose.

Purposes for stream ``c`` at the absolute step ``s`` (key = seed low / high word, counter = step low, step high, stream, purpose):
  0  selection   molecule ``min(floor(U(w0, w1) nmol), nmol - 1)``; a rotation iff the molecule has more than one atom and
                 ``U(w2, w3) < p_rotation``
  1, 2 geometry  translation (``random_translation``, mcmoves.jl:139-146): ``r = (2U - 1) dmax`` per axis from (w0, w1), (w2, w3)
                 of purpose 1 and (w0, w1) of purpose 2; rotation (``random_rotation``, :147-164): ``theta = thetamax (2 U(w0, w1) - 1)``,
                 axis ``min(floor(3 U(w2, w3)), 2)`` of purpose 1, about atom ``bead``
  3  acceptance  ``u = U(w0, w1)``
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF

SELECT, GEOMETRY_A, GEOMETRY_B, ACCEPT = 0, 1, 2, 3
TRANSLATION, ROTATION = 0, 1


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
