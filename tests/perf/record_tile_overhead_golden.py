"""Record the golden files of tests/test_gpu_tile_overhead.py: every stored Float32 grid and every raw FP64 sum of the cases of
tests/tile_overhead_cases.py, from the library CEG_HIP_LIB names (default: the one in the tree), into
tests/golden/tile_overhead/<case>.npz (or the directory given as first argument).  Needs a GPU.

    CEG_HIP_LIB=/path/to/the/parent/libceg_hip.so python tests/perf/record_tile_overhead_golden.py [outdir]

The files in the repository were recorded from the library of the commit BEFORE the bookkeeping of k_culled was rewritten: the test
asserts that nothing the kernel stores has changed since."""
import os
import sys
from pathlib import Path

import numpy as np

root = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(root / "crystalenergygrids.jl_amd"), str(root), str(root / "tests")]
import torch  # noqa: F401,E402  (before the library: see tests/conftest.py)
import tile_overhead_cases as TC  # noqa: E402

outdir = Path(sys.argv[1]) if len(sys.argv) > 1 else TC.GOLDEN_DIR
outdir.mkdir(parents=True, exist_ok=True)
print("library:", os.environ.get("CEG_HIP_LIB", "(in tree)"))
for case in TC.all_cases():
    arrays = TC.run_case(case)
    np.savez_compressed(outdir / (case.slug + ".npz"), **arrays)
    print(f"{case.name}: {len(arrays)} arrays, {(outdir / (case.slug + '.npz')).stat().st_size} B", flush=True)
