"""The host side of the recorder of a chain group (ceg_mc_group_set_recorder, include/ceg_hip.h): the restatements in ceg_hip.mcrng of
the frame schedule and of the minimum rule against hand-computed cases, the layouts of the two structures against the header's text,
and the declarations of the five calls in the header, the ctypes table, the Julia shim and the Makefile.  No GPU."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from ceg_hip import _abi, mcrng


def test_snapshot_due_and_cycles():
    # every = 0: never
    assert not any(mcrng.snapshot_due(cc, 0, 0) for cc in range(0, 20)) and mcrng.snapshot_cycles(1, 50, 0, 0) == []
    # origin = 0, every = 1: every cycle of the call
    assert mcrng.snapshot_cycles(1, 4, 0, 1) == [1, 2, 3, 4]
    # every = 3 from origin = 4: 4, 7, 10, ...; nothing before the origin
    assert [cc for cc in range(0, 14) if mcrng.snapshot_due(cc, 4, 3)] == [4, 7, 10, 13]
    assert mcrng.snapshot_cycles(1, 12, 4, 3) == [4, 7, 10]
    # origin beyond the run: none; origin on the last cycle: that one
    assert mcrng.snapshot_cycles(1, 12, 13, 1) == [] and mcrng.snapshot_cycles(1, 12, 12, 5) == [12]
    # a later call: cycle0 = 9 > origin = 4 and (9 - 4) % 3 == 2, so the first frame is cycle 10
    assert mcrng.snapshot_cycles(9, 8, 4, 3) == [10, 13, 16] and mcrng.snapshot_cycles(11, 2, 4, 3) == []
    # the reference's idx_cycle % printevery == 0 with ninit = 2, printevery = 5, cycle0 counted from 1: idx_cycle = cc - ninit
    assert mcrng.snapshot_cycles(1, 14, 2, 5) == [2, 7, 12]
    assert mcrng.snapshot_cycles(5, 0, 0, 1) == []
    with pytest.raises(ValueError):
        mcrng.snapshot_due(3, -1, 1)
    with pytest.raises(ValueError):
        mcrng.snapshot_due(3, 0, -1)


def test_track_minimum():
    nan = math.nan
    #            chain 0   1      2     3      4
    E = np.array([[5.0, -1.0, 3.0, 2.0, nan],          # cycle 1
                  [4.0, -1.0, 1.0, 9.0, nan],          # cycle 2
                  [4.0, -3.0, nan, 1.0, 8.0],          # cycle 3
                  [6.0, -3.0, 0.5, 0.0, 7.5]])         # cycle 4
    e0 = [4.5, -1.0, 2.0, 1.5, 7.5]
    stopped = np.zeros(E.shape, dtype=bool)
    stopped[2:, 3] = True                              # chain 3 is stopped from the end of cycle 3 on
    mink, mine = mcrng.track_minimum(E, e0, stopped)
    # chain 0: 4.0 first at cycle 2, the tie at cycle 3 keeps cycle 2.  chain 1: the tie with e0 keeps -1 until -3.0 at cycle 3 (not 4).
    # chain 2: the NaN at cycle 3 never wins, 0.5 at cycle 4.  chain 3: stopped before its 1.0 and 0.0: e0 stays.  chain 4: NaN, NaN,
    # 8.0 > e0, 7.5 == e0 is no strict <: e0 stays.
    assert list(mink) == [2, 3, 4, -1, -1] and list(mine) == [4.0, -3.0, 0.5, 1.5, 7.5]
    assert mink.dtype == np.int64 and mine.dtype == np.float64
    # without `stopped` chain 3 goes on to cycle 4; cycle0 shifts the cycle numbers
    mink, mine = mcrng.track_minimum(E, e0, cycle0=11)
    assert list(mink) == [12, 13, 14, 14, -1] and mine[3] == 0.0
    # a NaN start never loses either: `e < NaN` is false
    mink, mine = mcrng.track_minimum([[1.0]], [nan])
    assert list(mink) == [-1] and math.isnan(mine[0])
    mink, mine = mcrng.track_minimum(np.zeros((0, 2)), [1.0, 2.0])
    assert list(mink) == [-1, -1] and list(mine) == [1.0, 2.0]


def test_layouts_and_declarations():
    assert C.sizeof(_abi.McRecorder) == 48 and _abi.MC_SNAPSHOT_RECORD_DTYPE.itemsize == 40
    R = _abi.McRecorder
    assert [getattr(R, n).offset for n in ("every", "origin", "frame_capacity", "max_atoms", "max_molecules", "track_min", "_pad", "energy")] == \
        [0, 8, 16, 24, 28, 32, 36, 40]
    f = _abi.MC_SNAPSHOT_RECORD_DTYPE.fields
    assert [f[n][1] for n in ("cycle", "step", "energy", "nmol", "natoms", "flags", "_pad")] == [0, 8, 16, 24, 28, 32, 36]
    header = (_abi.REPO_DIR / "include" / "ceg_hip.h").read_text()

    def names(body):
        return [n for decl in re.findall(r"(?:int32_t|int64_t|double|const double\*)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]

    m = re.search(r"typedef struct ceg_mc_recorder \{\s*/\* 48 bytes \*/(.*?)\} ceg_mc_recorder_t;", header, re.S)
    assert m and names(m.group(1)) == [n for n, _t in _abi.McRecorder._fields_]
    m = re.search(r"typedef struct ceg_mc_snapshot_record \{\s*/\* 40 bytes \*/(.*?)\} ceg_mc_snapshot_record_t;", header, re.S)
    assert m and names(m.group(1)) == list(_abi.MC_SNAPSHOT_RECORD_DTYPE.names)
    m = re.search(r"#define\s+CEG_MC_RECORDER_MAX_BYTES\s+\(\(int64_t\)8 << 30\)", header)
    assert m and _abi.MC_RECORDER_MAX_BYTES == 8 << 30
    arity = {"ceg_mc_group_set_recorder": 2, "ceg_mc_group_snapshot": 1, "ceg_mc_group_recorder_rebase": 2, "ceg_mc_group_recorder_read": 9,
             "ceg_mc_group_recorder_min": 8}
    julia = (_abi.PKG_DIR / "julia" / "CEGHip.jl").read_text()
    for name, n in arity.items():
        assert re.search(r"CEG_API\s+int\s+" + name + r"\s*\(", header), name
        assert len(_abi.PROTOTYPES[name][1]) == n, name
    for name in ("ceg_mc_group_set_recorder", "ceg_mc_group_snapshot", "ceg_mc_group_recorder_read", "ceg_mc_group_recorder_min"):
        assert f"(:{name}, LIB[])" in julia, name
    for name in ("mc_group_set_recorder!", "mc_group_snapshot!", "mc_group_recorder_read", "mc_group_recorder_min"):
        assert f"function {name}(" in julia, name
    assert "ceg_mc_record.hip" in (_abi.PKG_DIR / "csrc" / "Makefile").read_text()
    # the three remarks that snapshots are not covered are gone
    for text in (header, (_abi.REPO_DIR / "DESIGN.md").read_text(), (_abi.REPO_DIR / "INTEGRATION.md").read_text()):
        for m in re.finditer(r"Not covered:(.*?)(?:\*/|\n\n)", text, re.S):
            assert "snapshot" not in m.group(1), m.group(0)[:200]


def test_the_methods_exist():
    from ceg_hip.energy import DeviceMonteCarloGroup
    for name in ("set_recorder", "snapshot", "recorder_rebase", "recorder_read", "recorder_minimum", "restore"):
        assert callable(getattr(DeviceMonteCarloGroup, name)), name
