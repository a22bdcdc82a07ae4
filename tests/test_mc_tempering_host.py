"""The host restatement of the replica exchange of ceg_mc_group_set_tempering (ceg_hip.mcrng: exchange_pairs, exchange_threshold,
exchange_round) on values worked out by hand: the pairs of a round, the rule of run_parallel_tempering (simulation.jl:533) in the
operation order of k_mcg_exchange, and one five-chain cycle end.  No device needed; tests/test_gpu_mc_tempering.py holds the device to
this module."""
import ctypes as C
import math
import re
from fractions import Fraction

import numpy as np

from ceg_hip import _abi, mcrng


def test_pairs_of_a_round():
    """K = 1, 2, 5 at both parities with every = 1 and 3; no round where cc % every != 0"""
    for every in (1, 3):
        even, odd = 2 * every, 1 * every           # (cc / every) & 1 == 0, 1
        assert mcrng.exchange_pairs(1, even, every) == [] and mcrng.exchange_pairs(1, odd, every) == []
        assert mcrng.exchange_pairs(2, even, every) == [(0, 1)] and mcrng.exchange_pairs(2, odd, every) == []
        assert mcrng.exchange_pairs(5, even, every) == [(0, 1), (2, 3)] and mcrng.exchange_pairs(5, odd, every) == [(1, 2), (3, 4)]
    for cc in (1, 2, 4, 5, 7, 8):
        assert mcrng.exchange_pairs(5, cc, 3) == []
    assert mcrng.exchange_pairs(5, 3, 3) == [(1, 2), (3, 4)] and mcrng.exchange_pairs(5, 6, 3) == [(0, 1), (2, 3)] and mcrng.exchange_pairs(5, 9, 3) == [(1, 2), (3, 4)]
    assert mcrng.exchange_pairs(6, 1, 1) == [(1, 2), (3, 4)] and mcrng.exchange_pairs(6, 2, 1) == [(0, 1), (2, 3), (4, 5)]
    assert mcrng.EXCHANGE == 9


def _nearest(x: Fraction) -> float:
    """the FP64 nearest to the rational x (Python's int / int division is correctly rounded)"""
    return x.numerator / x.denominator


def _threshold_exponent(Ea, Eb, Ta, Tb) -> float:
    """x of the rule from exact rational arithmetic, rounded to FP64 after every operation"""
    ia = _nearest(Fraction(1) / Fraction(Ta))
    ib = _nearest(Fraction(1) / Fraction(Tb))
    d = _nearest(Fraction(ia) - Fraction(ib))
    Tp = _nearest(Fraction(1) / Fraction(d))
    return _nearest((Fraction(Ea) - Fraction(Eb)) / Fraction(Tp))


def test_threshold_against_exact_arithmetic_rounded_per_step():
    cases = [(-1500.0, -1400.0, 300.0, 400.0), (-1400.0, -1500.0, 300.0, 400.0), (-25000.5, -24990.25, 200.0, 230.0), (10.0, 250.0, 450.0, 600.0),
             (-3.0e5, -3.0e5 + 7.0, 299.0, 301.0), (0.1, 0.3, 0.7, 1.9)]
    for Ea, Eb, Ta, Tb in cases:
        x = _threshold_exponent(Ea, Eb, Ta, Tb)
        assert mcrng.exchange_threshold(Ea, Eb, Ta, Tb) == math.exp(x), (Ea, Eb, Ta, Tb)
    # by hand: 1/300 - 1/400 = 1/1200, Tp = 1200, x = -100 / 1200
    x = _threshold_exponent(-1500.0, -1400.0, 300.0, 400.0)
    assert abs(Fraction(x) + Fraction(1, 12)) < Fraction(1, 10 ** 14)
    assert abs(mcrng.exchange_threshold(-1500.0, -1400.0, 300.0, 400.0) - 0.9200444146293233) < 1e-15
    assert mcrng.exchange_threshold(-1400.0, -1500.0, 300.0, 400.0) > 1.0        # downhill for the pair: always accepted
    # the order matters: (E_a - E_b) / Tp, not (E_a - E_b) * d
    assert mcrng.exchange_threshold(-25000.5, -24990.25, 200.0, 230.0) == math.exp((-25000.5 - -24990.25) / (1.0 / (1.0 / 200.0 - 1.0 / 230.0)))


def test_threshold_at_equal_temperatures_and_with_nan():
    for E in ((-100.0, 50.0), (50.0, -100.0), (0.0, 0.0), (1e300, -1e300)):
        assert mcrng.exchange_threshold(E[0], E[1], 350.0, 350.0) == 1.0
        assert mcrng.exchange_rule(E[0], E[1], 0.999999, mcrng.exchange_threshold(E[0], E[1], 350.0, 350.0))
    for Ea, Eb in ((math.nan, 1.0), (1.0, math.nan), (math.nan, math.nan)):
        e = mcrng.exchange_threshold(Ea, Eb, 300.0, 400.0)
        assert math.isnan(e) and not mcrng.exchange_rule(Ea, Eb, 0.0, e)
    assert mcrng.exchange_threshold(1e6, -1e6, 1.0, 2.0) == math.inf and mcrng.exchange_threshold(-1e6, 1e6, 1.0, 2.0) == 0.0


def test_threshold_of_the_reverse_pair_is_the_reciprocal():
    rng = np.random.default_rng(7)
    for _ in range(200):
        Ea, Eb = rng.uniform(-3e4, -1e4, 2)
        Ta = rng.uniform(200.0, 500.0)
        Tb = Ta + rng.uniform(1.0, 100.0)
        p = mcrng.exchange_threshold(Ea, Eb, Ta, Tb) * mcrng.exchange_threshold(Eb, Ea, Ta, Tb)
        # x and -x are exact negatives (every step is sign-symmetric); exp(x) exp(-x) is 1 to three roundings
        assert abs(p - 1.0) <= 4 * 2.0 ** -52, (Ea, Eb, Ta, Tb, p)


def test_a_round_of_five_chains_written_out_by_hand():
    """cc = 4, every = 2: parity 0, pairs (0, 1) and (2, 3); rung 4 is in no pair.  rung = [2, 0, 4, 1, 3]: rung 0 holds chain 1, rung 1
    chain 3, rung 2 chain 0, rung 3 chain 4, rung 4 chain 2.  Pair (0, 1) = chains (1, 3): E_b < E_a, accepted whatever the draw.
    Pair (2, 3) = chains (0, 4): chain 4 is stopped, no attempt."""
    rung = [2, 0, 4, 1, 3]
    E = [-1200.0, -1000.0, -900.0, -1100.0, -1300.0]
    T, Tn = [300.0, 350.0, 400.0, 450.0, 500.0], [310.0, 360.0, 410.0, 460.0, 510.0]
    sid = [11, 12, 13, 14, 15]
    seed, step = 2024, 2 ** 33 + 17
    new, rec = mcrng.exchange_round(rung, E, T, [False, False, False, False, True], seed, step, sid, 4, 2, Tn)
    assert rec.dtype == _abi.MC_EXCHANGE_RECORD_DTYPE
    w = mcrng.draw(seed, step, 12, 9)                                    # the stream of chain 1, the lower chain of pair (0, 1)
    u = mcrng.uniform(w[0], w[1])
    e = math.exp((-1000.0 - -1100.0) / (1.0 / (1.0 / 300.0 - 1.0 / 350.0)))
    assert list(new) == [2, 1, 4, 0, 3]
    want = [(2, 2, -1, -1, -1200.0, 410.0, 0.0, 0.0), (0, 1, 3, 1, -1000.0, 360.0, u, e), (4, 4, -1, -1, -900.0, 510.0, 0.0, 0.0),
            (1, 0, 1, 1, -1100.0, 310.0, u, e), (3, 3, -1, -1, -1300.0, 460.0, 0.0, 0.0)]
    assert [tuple(r) for r in rec.tolist()] == want
    # the same round at the other parity: pairs (1, 2) = chains (3, 0) and (3, 4) = chains (4, 2), the latter with the stopped chain.
    # Chains (3, 0): E_a = -1100 > E_b = -1200, accepted.
    new, rec = mcrng.exchange_round(rung, E, T, [False, False, False, False, True], seed, step, sid, 6, 2)
    w = mcrng.draw(seed, step, 14, mcrng.EXCHANGE)
    assert list(new) == [1, 0, 4, 2, 3] and rec["u"][3] == rec["u"][0] == mcrng.uniform(w[0], w[1]) and list(rec["partner"]) == [3, -1, -1, 0, -1]
    assert list(rec["accepted"]) == [1, -1, -1, 1, -1] and list(rec["temperature_next"]) == [350.0, 300.0, 500.0, 400.0, 450.0]
    # uphill for the pair: the draw decides.  Chains (1, 3) with the energies exchanged: e < 1
    E2 = list(E)
    E2[1], E2[3] = E[3], E[1]
    new, rec = mcrng.exchange_round(rung, E2, T, [False] * 5, seed, step, sid, 4, 2)
    e = mcrng.exchange_threshold(-1100.0, -1000.0, 300.0, 350.0)
    assert 0.0 < e < 1.0 and rec["threshold"][1] == rec["threshold"][3] == e and rec["accepted"][1] == int(u < e) and rec["u"][1] == u
    assert list(rec["partner"]) == [4, 3, -1, 1, 0] and rec["accepted"][0] == rec["accepted"][4] != -1
    # no round: nothing moves, every chain gets its record
    new, rec = mcrng.exchange_round(rung, E, T, [False] * 5, seed, step, sid, 5, 2, Tn)
    assert list(new) == rung and (rec["accepted"] == -1).all() and (rec["partner"] == -1).all() and list(rec["temperature_next"]) == [Tn[r] for r in rung]


def test_layouts_and_declarations():
    assert C.sizeof(_abi.McTempering) == 32 and _abi.MC_EXCHANGE_RECORD_DTYPE.itemsize == 48
    f = _abi.MC_EXCHANGE_RECORD_DTYPE.fields
    assert [f[n][1] for n in ("rung", "rung_next", "partner", "accepted", "energy", "temperature_next", "u", "threshold")] == [0, 4, 8, 12, 16, 24, 32, 40]
    T = _abi.McTempering
    assert (T.every.offset, T.record_capacity.offset, T.rung.offset, T.energy.offset) == (0, 8, 16, 24)
    header = (_abi.REPO_DIR / "include" / "ceg_hip.h").read_text()
    m = re.search(r"typedef struct ceg_mc_tempering \{\s*/\* 32 bytes \*/(.*?)\} ceg_mc_tempering_t;", header, re.S)
    assert m and re.findall(r"(\w+);", m.group(1)) == ["every", "record_capacity", "rung", "energy"]
    m = re.search(r"typedef struct ceg_mc_exchange_record \{\s*/\* 48 bytes \*/(.*?)\} ceg_mc_exchange_record_t;", header, re.S)
    names = [n for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", m.group(1)) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == list(_abi.MC_EXCHANGE_RECORD_DTYPE.names)
    assert re.search(r"CEG_API\s+int\s+ceg_mc_group_set_tempering\s*\(", header) and len(_abi.PROTOTYPES["ceg_mc_group_set_tempering"][1]) == 2
    assert re.search(r"CEG_API\s+int\s+ceg_mc_group_tempering_read\s*\(", header) and len(_abi.PROTOTYPES["ceg_mc_group_tempering_read"][1]) == 6
    philox = (_abi.PKG_DIR / "csrc" / "ceg_philox.h").read_text()
    assert re.search(r"EXCHANGE\s*=\s*9\b", philox)
    julia = (_abi.PKG_DIR / "julia" / "CEGHip.jl").read_text()
    assert "(:ceg_mc_group_set_tempering, LIB[])" in julia and "(:ceg_mc_group_tempering_read, LIB[])" in julia
    assert "ceg_mc_temper.hip" in (_abi.PKG_DIR / "csrc" / "Makefile").read_text()
