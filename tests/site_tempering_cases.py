"""Tempering ladders on the synthetic site-hopping tables of tests/site_cases.py, shared by tests/test_site_tempering_host.py (CPU) and
tests/test_gpu_site_tempering.py (GPU).  A case is (n sites, m molecules, R rungs, L ladders); K = L * R chains, chain l * R + r is
rung r of ladder l.  Populations, streams, the seed and the ``first_step`` that crosses 2^32 inside the run are those of site_cases.

The host replay of a case (``mcrng.site_ladder_replay`` from the extended-precision baseline) is computed once and kept."""
import functools

import numpy as np

import site_cases as SC
from ceg_hip import mcrng

# the smallest ladder; m just under a wave; R = 16, a full 1024-thread workgroup; a tail past the wave and several ladders;
# two strides and a tail at the reference's p = 0.1
CASES = ((5, 2, 2, 1), (70, 63, 3, 2), (70, 64, 16, 1), (200, 65, 5, 3), (300, 130, 4, 2))


def ncycles(case) -> int:
    return 12 if case[1] == 2 else (3 if case[1] >= 130 else 4)


def pair_cdf(case) -> np.ndarray:
    """p = 0.3 (the geometric table of the reference's schedule), the reference's own p = 0.1 at m = 130, and a uniform table for the
    16 rungs: the geometric one never reaches the top pairs in so short a run"""
    n, m, R, L = case
    if R == 16:
        return (np.arange(R - 1) + 1) * 0.5 / (R - 1)
    return mcrng.site_exchange_cdf(R, 0.1 if m == 130 else 0.3)


def temperatures(case) -> np.ndarray:
    """[K]: every ladder geometric from 300 K to 600 K, the 16 rungs from 200 K to 2000 K"""
    n, m, R, L = case
    lo, hi = (200.0, 2000.0) if R == 16 else (300.0, 600.0)
    return np.tile(lo * (hi / lo) ** (np.arange(R) / (R - 1)), L)


def ladder_streams(case) -> np.ndarray:
    """(1012: among the first streams above 1000, one on which even the 24 steps of the smallest case hold every kind of exchange
    that tests/test_site_tempering_host.py asks for -- chosen by the host replay, which is what the device is then held to)"""
    return (1012 + 5 * np.arange(case[3])).astype(np.uint32)


def replay_ladder(case, l: int, nc=None, start_energy=None, log=None, first=None, cdf=None):
    """ladder ``l`` of the case through ``nc`` cycles of m steps; ``log`` [steps, R]: the ladder's columns of a device log"""
    n, m, R, L = case
    nc = ncycles(case) if nc is None else nc
    fw, it = SC.tables(n)
    rows = slice(l * R, (l + 1) * R)
    pops = SC.populations(n, m, L * R)[rows]
    e0 = [float(mcrng.site_baseline(fw, it, p)) for p in pops] if start_energy is None else [float(e) for e in start_energy]
    T = np.tile(temperatures(case)[rows], (nc, 1))
    return mcrng.site_ladder_replay(fw, it, pops, e0, SC.SEED, SC.first_step(m, nc) if first is None else first, SC.stream_ids(L * R)[rows],
                                    int(ladder_streams(case)[l]), T, m, pair_cdf(case) if cdf is None else cdf, log=log)


@functools.lru_cache(maxsize=None)
def host_replay(case):
    """[L] SiteLadderReplay by the rule on the host alone (no device log)"""
    return tuple(replay_ladder(case, l) for l in range(case[3]))


def exchanges(rp, m: int):
    """-> list of (step index t, pair j, SiteStep) of one ladder's replay, from the records of the lower rungs"""
    out = []
    for j, steps in enumerate(rp.steps):
        out += [(t, j, st) for t, st in enumerate(steps) if st.molecule == -1]
    return sorted(out, key=lambda x: x[0])


def coverage(rp, m: int) -> dict:
    """what the exchanges of one ladder reach: outcomes, neighbours in time, places in the cycle, near-ties"""
    ex = exchanges(rp, m)
    at = {t for t, _j, _s in ex}
    out = dict(downhill=0, drawn=0, rejected=0, consecutive=0, first=0, last=0, near_ties=0, pairs=set())
    for t, j, st in ex:
        down = st.after < st.before
        out["downhill"] += down and st.accepted
        out["drawn"] += (not down) and st.accepted
        out["rejected"] += not st.accepted
        out["consecutive"] += (t + 1) in at
        out["first"] += t % m == 0
        out["last"] += t % m == m - 1
        out["near_ties"] += (not down) and abs(st.u - st.threshold) < 1e-12
        out["pairs"].add(j)
    return out
