"""The host restatement of the cycle end of ceg_mc_group_sweep_cycles / ceg_mc_group_sweep_gcmc_cycles (ceg_hip.mcrng: adapt_dmax,
adapt_thetamax, cycle_records) on values worked out by hand: the adaptation of statistics.dmax / statistics.θmax at the end of a cycle
of run_montecarlo! (simulation.jl:818-827), thetamax in radians.  No device needed; tests/test_gpu_mc_cycles.py holds the device to
this module."""
import ctypes as C
import math
import re
from fractions import Fraction

import numpy as np

from ceg_hip import _abi, mcrng

DEG = math.pi / 180.0


def test_hand_checked_values():
    assert mcrng.adapt_dmax(1.3, 3, 8, 1) == 1.351387011977736
    assert mcrng.adapt_dmax(1.3, 0, 5, 1) == 1.1972259760445276
    assert mcrng.adapt_dmax(2.9, 9, 10, 3) == 3.0
    assert mcrng.adapt_dmax(0.1, 0, 7, 2) == 0.1
    assert mcrng.adapt_thetamax(0.5235987755982988, 3, 8, 1) == 0.2617993877991494
    assert mcrng.adapt_thetamax(0.5235987755982988, 5, 5, 2) == 1.0471975511965976
    assert mcrng.adapt_thetamax(0.2, 0, 4, 1) == 0.17453292519943295


def test_the_constants_are_the_reference_s_degrees():
    assert mcrng.THETAMAX_MIN == 10.0 * DEG and mcrng.THETAMAX_MAX == math.pi and mcrng.THETAMAX_GAIN == 2.0 * math.pi / 3.0
    assert (mcrng.DMAX_MIN, mcrng.DMAX_MAX) == (0.1, 3.0)
    # the operation order, once, against exact rational arithmetic rounded at every step
    r = 3.0 / 8.0
    q = 10.0 / 100.0
    s = math.sqrt(q)
    assert mcrng.adapt_dmax(1.3, 3, 8, 1) == 1.3 * (1.0 + (r - 0.25) * s)
    assert abs(Fraction(mcrng.adapt_dmax(1.3, 3, 8, 1)) - Fraction(13, 10) * (1 + Fraction(1, 8) * Fraction(s))) < Fraction(1, 10 ** 15)


def test_zero_trials_leave_the_value_unchanged():
    """the reference's NaN ratio (simulation.jl:819,824)"""
    for cc in (1, 7, 10 ** 6):
        assert mcrng.adapt_dmax(1.2345, 0, 0, cc) == 1.2345
        assert mcrng.adapt_thetamax(0.777, 0, 0, cc) == 0.777
    # also outside the clamps: nothing is touched
    assert mcrng.adapt_dmax(5.0, 0, 0, 1) == 5.0 and mcrng.adapt_thetamax(0.01, 0, 0, 1) == 0.01


def test_both_clamps_of_both_quantities():
    assert mcrng.adapt_dmax(2.99, 10, 10, 1) == 3.0                   # 2.99 * (1 + 0.75 sqrt(0.1)) > 3
    assert mcrng.adapt_dmax(0.1001, 0, 10, 1) == 0.1                  # 0.1001 * (1 - 0.25 sqrt(0.1)) < 0.1
    assert mcrng.adapt_thetamax(3.0, 10, 10, 1) == math.pi            # 3 + 0.5 * 120 deg > 180 deg
    assert mcrng.adapt_thetamax(0.2, 0, 10, 1) == 10.0 * DEG          # 0.2 - 0.5 * 120 deg < 10 deg
    # a value that starts outside is brought to the nearer bound
    assert mcrng.adapt_dmax(7.0, 1, 4, 1) == 3.0 and mcrng.adapt_dmax(0.01, 1, 4, 1) == 0.1
    # exactly at the target ratios nothing moves
    assert mcrng.adapt_dmax(1.7, 1, 4, 5) == 1.7 and mcrng.adapt_thetamax(1.1, 2, 4, 5) == 1.1


def test_a_large_cycle_counter():
    cc = 10 ** 6
    s = math.sqrt(10.0 / float(99 + cc))
    assert mcrng.adapt_dmax(1.3, 1, 1, cc) == 1.3 * (1.0 + 0.75 * s) and 1.3 < mcrng.adapt_dmax(1.3, 1, 1, cc) < 1.3 * 1.0024
    assert mcrng.adapt_thetamax(1.0, 1, 1, cc) == 1.0 + (0.5 / 1e6) * mcrng.THETAMAX_GAIN
    assert mcrng.adapt_thetamax(1.0, 0, 1, cc) == 1.0 + (-0.5 / 1e6) * mcrng.THETAMAX_GAIN


def test_cycle_records_against_a_three_cycle_table():
    """One chain, three cycles of 8 steps from cycle0 = 1 with nothing before: the call's counters after each cycle written by hand;
    the chain is empty at the end of the third cycle, which carries both values over."""
    counters = [(5, 2, 3, 3), (9, 2, 7, 4), (12, 5, 12, 4)]
    rec = mcrng.cycle_records([300.0, 450.0, 600.0], 1.3, 30.0 * DEG, counters, [6, 6, 0], [-1.5, -2.25, 4.0], [0.0, 10.0, 10.0])
    d1 = 1.3 * (1.0 + (2.0 / 5.0 - 0.25) * math.sqrt(10.0 / 100.0))
    t1 = 30.0 * DEG + ((3.0 / 3.0 - 0.5) / 1.0) * mcrng.THETAMAX_GAIN
    d2 = d1 * (1.0 + (2.0 / 9.0 - 0.25) * math.sqrt(10.0 / 101.0))
    t2 = t1 + ((4.0 / 7.0 - 0.5) / 2.0) * mcrng.THETAMAX_GAIN
    want = [(300.0, 1.3, 30.0 * DEG, d1, t1, -1.5, 0.0, 5, 2, 3, 3, 6, 0),
            (450.0, d1, t1, d2, t2, -2.25, 10.0, 9, 2, 7, 4, 6, 0),
            (600.0, d2, t2, d2, t2, 4.0, 10.0, 12, 5, 12, 4, 0, 0)]
    assert rec.dtype == _abi.MC_CYCLE_RECORD_DTYPE and [tuple(r) for r in rec.tolist()] == want
    assert 0.1 < d2 < d1 < 3.0 and 10.0 * DEG < t1 < t2 < math.pi
    # the adapt bits one by one, and a continuation: cycles 2 and 3 from the first record equal the one-call run
    only_d = mcrng.cycle_records([300.0] * 3, 1.3, 0.5, counters, [6] * 3, adapt=mcrng.ADAPT_DMAX)
    only_t = mcrng.cycle_records([300.0] * 3, 1.3, 0.5, counters, [6] * 3, adapt=mcrng.ADAPT_THETAMAX)
    none = mcrng.cycle_records([300.0] * 3, 1.3, 0.5, counters, [6] * 3, adapt=0)
    assert (only_d["thetamax_next"] == 0.5).all() and only_d["dmax_next"][0] == d1 and (only_t["dmax_next"] == 1.3).all()
    assert (none["dmax_next"] == 1.3).all() and (none["thetamax_next"] == 0.5).all()
    prior = counters[0]
    rest = [tuple(x - p for x, p in zip(c, prior)) for c in counters[1:]]
    cont = mcrng.cycle_records([450.0, 600.0], d1, t1, rest, [6, 0], [-2.25, 4.0], [10.0, 10.0], cycle0=2, prior=prior)
    assert cont.tobytes() == rec[1:].tobytes()


def test_layouts_and_declarations():
    assert C.sizeof(_abi.McCycles) == 48 and _abi.MC_CYCLE_RECORD_DTYPE.itemsize == 96
    f = _abi.MC_CYCLE_RECORD_DTYPE.fields
    assert [f[n][1] for n in ("temperature", "dmax_next", "delta_moves", "translation_trials", "rotation_accepted", "nmol")] == [0, 24, 40, 56, 80, 88]
    assert (_abi.McCycles.adapt.offset, _abi.McCycles.temperatures.offset, _abi.McCycles.prior.offset) == (24, 32, 40)
    assert (_abi.MC_ADAPT_DMAX, _abi.MC_ADAPT_THETAMAX) == (mcrng.ADAPT_DMAX, mcrng.ADAPT_THETAMAX) == (1, 2)
    header = (_abi.REPO_DIR / "include" / "ceg_hip.h").read_text()
    for name in ("ceg_mc_group_sweep_cycles", "ceg_mc_group_sweep_gcmc_cycles"):
        assert re.search(r"CEG_API\s+int\s+" + name + r"\s*\(", header), name
        assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name][1]) == 6
    assert "#define CEG_MC_ADAPT_DMAX     1" in header and "#define CEG_MC_ADAPT_THETAMAX 2" in header
    assert f"#define CEG_MC_CYCLES_MAX_RECORDS {_abi.MC_CYCLES_MAX_RECORDS}" in header
