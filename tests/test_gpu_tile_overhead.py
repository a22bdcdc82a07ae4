"""GPU tests of the bookkeeping of the grid kernel outside its pair loops (k_culled: tile box from the two corner lanes in grid
mode, row-count scan on DPP, flat index -> bin row through a scattered map and a max-scan): nothing that is stored may change.

Every launch of every case of ``tests/tile_overhead_cases.py`` -- partial tiles on each axis, thin grids, x ranges, launches whose
last workgroup has idle waves, a sparse framework (empty bin rows between non-empty ones), a dense one at a 21 A cutoff (several
row passes, tens of chunks), three cutoffs on one cell, and one launch per code shape (fused class 1 / 2, VdW-only, Coulomb-only,
Buckingham, two probes, point lists) -- is compared

  * bit for bit with ``tests/golden/tile_overhead/<case>.npz``, recorded with ``tests/perf/record_tile_overhead_golden.py`` from
    the library of the commit before the rewrite (stored Float32 grids; raw FP64 sums of the POINTS launches), and
  * with the CPU oracle at the suite's tolerances (``compare_grids`` / ``compare_raw`` defaults), so that a wrong golden file
    cannot hide.

``tests/test_tile_overhead_cases_host.py`` asserts on the CPU that the cases contain what they are meant to."""
import numpy as np
import pytest

from oracle.compare import compare_grids

import tile_overhead_cases as TC
from util import compare_raw

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("case", TC.all_cases(), ids=lambda c: c.name)
def test_stored_values_are_those_of_the_parent_commit(hip_lib, oracle, case):
    got = TC.run_case(case)
    with np.load(TC.GOLDEN_DIR / (case.slug + ".npz")) as z:
        golden = {k: z[k] for k in z.files}
    assert set(got) == set(golden)
    for name in sorted(got):
        g, ref = got[name], golden[name]
        assert g.dtype == ref.dtype and g.shape == ref.shape, name
        differ = _bits(g) != _bits(ref)
        print(f"{case.name} {name}: {int(differ.sum())} of {differ.size} values differ from the golden file")
        assert not differ.any(), f"{case.name} {name}: {int(differ.sum())} stored values differ from the parent commit's, first at {np.argwhere(differ)[0]}"
        launch, what = name.rsplit("/", 1)
        if launch == "points":
            worst = compare_raw(g, case.ref(oracle, "points_" + what), f"{case.name} {name} vs oracle")
        else:
            b, e = (int(x) for x in launch[launch.index("[") + 1:-1].split(","))
            worst = compare_grids(g, case.ref(oracle, what)[:, b:e], f"{case.name} {name} vs oracle")
        print(f"{case.name} {name}: worst relative error vs oracle {worst:.2e}")
