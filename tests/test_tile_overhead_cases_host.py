"""CPU-side assertions on the cases of ``tests/tile_overhead_cases.py`` (what ``tests/test_gpu_tile_overhead.py`` runs on the
device), so that the device test cannot pass vacuously: through the numpy mirror of the image bins and of the row pass the cases
contain an empty bin row between non-empty ones, tiles with more than 64 rows, rows that straddle a chunk boundary, partial tiles
on every axis, launches whose last workgroup has idle waves -- and every case has its golden file."""
import numpy as np
import pytest

from ceg_hip import _abi

import tile_overhead_cases as TC

CASES = TC.all_cases()
BY_NAME = {c.name: c for c in CASES}


def test_names_and_golden_files():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        f = TC.GOLDEN_DIR / (c.slug + ".npz")
        assert f.exists(), f"{f} is missing: record it with tests/perf/record_tile_overhead_golden.py"
        assert f.stat().st_size < 1 << 20
        with np.load(f) as z:
            names = set(z.files)
        want = set()
        for mode, b, e in c.launches:
            if mode == "points":
                want |= {"points/vdw", "points/coulomb"}
            else:
                outs = {"fused": ("vdw", "coulomb"), "vdw": ("vdw",), "coulomb": ("coulomb",), "multi": ("vdw", "vdw_q", "coulomb")}[mode]
                want |= {f"{mode}[{b},{e})/{o}" for o in outs}
        assert names == want, c.name


def test_partial_tiles_on_every_axis_and_thin_grids():
    rem = lambda ax: {c.npoints[ax] % 4 for c in CASES}
    for ax in range(3):
        assert rem(ax) >= {1, 2, 3}, ax                                  # 4n + 1, 4n + 2, 4n + 3 points
        assert any(c.npoints[ax] < 4 for c in CASES), ax
    one_axis = [c for c in CASES if c.name.startswith("shape/") and sum(n % 4 != 0 for n in c.npoints) == 1]
    assert len(one_axis) == 9
    assert any(all(n % 4 != 0 for n in c.npoints) for c in CASES)
    # x ranges: a start that is no multiple of 4 (stored from that plane), a one-plane slab
    r = [(b, e) for m, b, e in BY_NAME["ranges/class1"].launches if m != "points"]
    assert any(b % 4 and e - b > 4 for b, e in r) and any(e - b == 1 for b, e in r)


def test_code_shapes():
    modes = {m for c in CASES for m, _, _ in c.launches}
    assert modes == {"fused", "vdw", "coulomb", "multi", "points"}
    assert {c.uniform_class for c in CASES if any(m == "fused" for m, _, _ in c.launches)} == {0, 1, 2}
    assert BY_NAME["buckingham"].uniform is None and (BY_NAME["buckingham"].kinds == TC.B).any()
    assert {c.cutoff for c in CASES if c.name.startswith("cutoff/")} == {9.0, 10.5, 12.0}


@pytest.mark.parametrize("case", [c for c in CASES if c.name != "multi"], ids=lambda c: c.name)
def test_uniform_class_of_the_plan(case):
    lib = _abi.load_library()
    pv, _ = case.probes()
    ff = pv.forcefield
    rules, offsets = ff.rule_table(pv.probe)
    kinds = np.ascontiguousarray(case.kinds, dtype=np.int64)
    q = np.ascontiguousarray(case.q, dtype=np.float64)
    consts = np.full(4, np.nan)
    rc = lib.ceg_uniform_class(_abi.i64ptr(kinds), _abi.dptr(q), len(kinds), rules.ctypes.data, _abi.i32ptr(offsets), ff.nkinds,
                               case.cutoff ** 2, _abi.dptr(consts))
    assert rc == case.uniform_class


def test_idle_waves_in_the_last_workgroup():
    """tiles per launch against the 4 and 8 waves (= tiles) of a workgroup of k_culled"""
    counts = [n for c in CASES for n in TC.walk_stats(c)["tiles"]]
    assert any(n % 8 != 0 and n % 4 != 0 for n in counts)
    assert any(n < 8 for n in counts) and any(n > 16 for n in counts)          # one partly idle workgroup of 8; several workgroups


def test_sparse_case_has_empty_rows_between_non_empty_ones():
    st = TC.walk_stats(BY_NAME["sparse/30-atoms"])
    assert st["empty_between"] and st["max_chunks"] >= 1


def test_dense_case_has_several_row_passes_and_many_chunks():
    st = TC.walk_stats(BY_NAME["dense21"])
    assert st["max_rows"] > 64 and st["max_chunks"] >= 12 and st["straddle"]


def test_rows_straddle_chunk_boundaries_at_every_cutoff():
    for cutoff in ("9", "10.5", "12"):
        st = TC.walk_stats(BY_NAME[f"cutoff/{cutoff}"])
        assert st["straddle"] and st["max_chunks"] >= 2, cutoff
    assert any(TC.walk_stats(c)["start_on_boundary"] for c in CASES)          # a row that starts exactly at a chunk boundary
