"""Synthetic site-hopping cases shared by tests/test_site_hopping_host.py (CPU) and tests/test_gpu_site_sweep.py (GPU): symmetric
random tables with the diagonal at 1e100, duplicate-free populations, one temperature per chain spread over two decades, and a
``first_step`` that makes the step counter cross its low 32-bit word inside the run.  No framework is needed.

The host replay of a case (``mcrng.site_replay`` from the extended-precision baseline) is computed once and kept."""
import functools

import numpy as np

from ceg_hip import mcrng

# (n sites, m molecules, K chains): one molecule; a handful; m = 63, 64, 65 around the wave; 130 = two full strides and a tail
CASES = ((2, 1, 1), (5, 2, 3), (70, 63, 5), (70, 64, 4), (200, 65, 5), (300, 130, 9))
NCYCLES = 3
SEED = 0x5EED51735


def tables(n: int):
    """framework in [-1000, 0) K, interactions symmetric in [-300, 300) K with the diagonal at 1e100"""
    rng = np.random.default_rng(1000 + n)
    fw = -1000.0 * rng.random(n)
    a = 600.0 * rng.random((n, n)) - 300.0
    it = np.triu(a, 1)
    it = it + it.T
    it[np.arange(n), np.arange(n)] = 1e100
    return fw, np.ascontiguousarray(it)


def populations(n: int, m: int, k: int) -> np.ndarray:
    return np.stack([mcrng.site_random_population(SEED, 100 + c, n, m) for c in range(k)])


def temperatures(k: int) -> np.ndarray:
    """30 K .. 3000 K, geometric"""
    return 30.0 * 100.0 ** (np.arange(k) / max(k - 1, 1))


def first_step(m: int, ncycles: int = NCYCLES) -> int:
    """the counter crosses 2^32 after about half of the run"""
    return 2 ** 32 - max((ncycles * m) // 2, 1)


def stream_ids(k: int) -> np.ndarray:
    return (7 + 3 * np.arange(k)).astype(np.uint32)


def replay_chain(n, m, k, c, ncycles, start_energy=None, log=None, first=None, pops=None):
    fw, it = tables(n)
    p = populations(n, m, k)[c] if pops is None else pops
    e0 = float(mcrng.site_baseline(fw, it, p)) if start_energy is None else float(start_energy)
    T = np.full(ncycles, temperatures(k)[c])
    return mcrng.site_replay(fw, it, p, e0, SEED, first_step(m, ncycles) if first is None else first, int(stream_ids(k)[c]), T, m, log=log)


@functools.lru_cache(maxsize=None)
def host_replay(n: int, m: int, k: int, ncycles: int = NCYCLES):
    """[K] SiteReplay by the rule on the host alone (no device log), from the extended-precision baseline"""
    return tuple(replay_chain(n, m, k, c, ncycles) for c in range(k))


def coverage(steps, start_population):
    """-> dict of counts over one chain's steps: accepted, rejected, hops onto an occupied site, hops onto the own site"""
    pop = [int(x) for x in start_population]
    out = dict(accepted=0, rejected=0, occupied=0, own=0, occupied_accepted=0, own_rejected=0)
    for st in steps:
        occ = st.new_site in pop and st.new_site != st.old_site
        own = st.new_site == st.old_site
        out["accepted" if st.accepted else "rejected"] += 1
        out["occupied"] += occ
        out["own"] += own
        out["occupied_accepted"] += occ and st.accepted
        out["own_rejected"] += own and not st.accepted
        if st.accepted:
            pop[st.molecule] = st.new_site
    return out


def near_ties(steps) -> int:
    """steps whose decision hangs on the last bits of exp: |u - e| < 1e-12 with after >= before"""
    return sum(1 for st in steps if not st.after < st.before and abs(st.u - st.threshold) < 1e-12)


# the recorder's cases: frames on a population longer than one stride, the minimum where ties with it are common
FRAMES_CASE, FRAMES_NCYCLES, FRAMES_ORIGIN = (200, 65, 5), 7, 2
MINIMUM_CASE, MINIMUM_NCYCLES = (5, 2, 3), 12


def minimum_ties(cycle_energy, e0: float) -> int:
    """cycle ends whose energy EQUALS the running minimum without beating it (strict <: the earlier frame must stay)"""
    mine, ties = float(e0), 0
    for e in cycle_energy:
        if e < mine:
            mine = float(e)
        elif e == mine:
            ties += 1
    return ties
