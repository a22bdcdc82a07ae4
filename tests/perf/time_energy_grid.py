"""Timing of ``ceg_energy_grid`` (energy_grid for a polyatomic guest, all rotations in one device pass) against the composed route
it replaces: ``GpuEnergySetup.energy_points`` on host-generated positions, in chunks of iC planes that fit host memory.

Workload: CO2 in CHA_1.4_3b4eeb96, step 0.3 A (95^3 lattice points), 50 rotations from ``rotation_matrices`` on 10 fixed unit
vectors (non-linear form: 5 z-rotations each).  No block file (``blockfile=False``) on either route: the composed route tests the
blocking mask in a Python loop per placement, which would time the interpreter.  Both routes run in this process on the same
device; one warm-up, then the median of ``--repeats``.  ``--new-only`` runs the new route alone (for a kernel trace).

    python tests/perf/time_energy_grid.py [--step 0.3] [--repeats 5] [--new-only] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (str(ROOT / "crystalenergygrids.jl_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

import ceg_hip as ceg                                               # noqa: E402
from ceg_hip.energy import GpuEnergySetup                            # noqa: E402
from ceg_hip.hostmirror.lebedev import rotation_matrices             # noqa: E402

FP64_PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--planes", type=int, default=4, help="iC planes per chunk of the composed route")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    import torch
    golden = ROOT / "tests" / "golden" / "raspa"
    with tempfile.TemporaryDirectory() as tmp:
        raspa = Path(tmp) / "raspa"
        raspa.mkdir()
        for sub in ("forcefield", "molecules", "structures"):
            os.symlink(golden / sub, raspa / sub)
        ceg.setdir_RASPA(raspa)
        setup = ceg.setup_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021", "CO2", "TraPPE", blockfile=False)
    rng = np.random.default_rng(50)
    u = rng.normal(size=(10, 3))
    rots = rotation_matrices(u / np.linalg.norm(u, axis=1)[:, None], False)
    nrot = len(rots)
    mat = setup.framework.mat
    num = [int(math.floor(np.linalg.norm(mat[:, a]) / args.step)) + 1 for a in range(3)]
    steps = [mat[:, a] / num[a] for a in range(3)]
    base = np.asarray(setup.molecule.position, dtype=np.float64).reshape(-1, 3)
    nk = len(setup.ewald.kfactors)
    say(f"CO2 in CHA_1.4_3b4eeb96, step {args.step} A: lattice {num[0]} x {num[1]} x {num[2]}, {nrot} rotations, {nk} k-vectors, "
        f"{nrot * num[0] * num[1] * num[2]} elements; device {torch.cuda.get_device_name(0)}")
    gs = GpuEnergySetup(setup)

    def timed(fn, repeats):
        fn()                                                        # warm-up
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    new = {}

    def run_new():
        new["grid"] = gs.energy_grid_rotations(args.step, rots)
    t_new, all_new = timed(run_new, args.repeats)
    say(f"ceg_energy_grid, host output:   median {t_new * 1e3:10.1f} ms   ({', '.join(f'{t * 1e3:.1f}' for t in all_new)})")
    d_out = torch.empty(nrot * num[0] * num[1] * num[2], dtype=torch.float64, device="cuda:0")

    def run_dev():
        gs.energy_grid_rotations(args.step, rots, out_device_ptr=d_out.data_ptr())
        torch.cuda.synchronize()
    t_dev, all_dev = timed(run_dev, args.repeats)
    say(f"ceg_energy_grid, device output: median {t_dev * 1e3:10.1f} ms   ({', '.join(f'{t * 1e3:.1f}' for t in all_dev)})")
    # FP64 work the contraction kernel executes: per wave and step of 4 k-vectors 2 MFMA 16x16x4 per rotation tile
    tiles_a, nt, nkp = (num[0] + 15) // 16, (nrot + 15) // 16, (nk + 15) // 16 * 16
    flops = 2.0 * 16 * 16 * 4 * 2 * nt * (nkp // 4) * tiles_a * num[1] * num[2]
    say(f"contraction: {flops / 1e9:.1f} GFLOP executed ({2.0 * 2 * nk * nrot * num[0] * num[1] * num[2] / 1e9:.1f} useful); over the whole "
        f"device-output call that is {flops / t_dev / FP64_PEAK:.3f} of the FP64 peak of 78.6 TFLOP/s (kernel times: the trace below)")
    if not args.new_only:
        rp = np.einsum("rij,aj->rai", rots, base)
        iA, iB = np.meshgrid(np.arange(num[0]), np.arange(num[1]), indexing="ij")

        def run_old():
            out = np.empty((nrot, num[0], num[1], num[2]))
            for c0 in range(0, num[2], args.planes):
                cs = np.arange(c0, min(c0 + args.planes, num[2]))
                ofs = (iA[..., None, None] * steps[0] + iB[..., None, None] * steps[1]) + cs[None, None, :, None] * steps[2]
                pos = ofs[None, :, :, :, None, :] + rp[:, None, None, None, :, :]
                e = gs.energy_points(pos.reshape(-1, len(base), 3))
                out[:, :, :, c0:c0 + len(cs)] = (e[:, 0] + e[:, 1]).reshape(nrot, num[0], num[1], len(cs))
            new["old"] = out
        t_old, all_old = timed(run_old, args.repeats)
        say(f"composed route (energy_points):  median {t_old * 1e3:10.1f} ms   ({', '.join(f'{t * 1e3:.1f}' for t in all_old)})")
        say(f"ratio new / composed = {t_new / t_old:.4f}   (required <= 0.95)")
        a, b = new["grid"], new["old"]
        say(f"largest |new - composed| / max|composed| = {np.abs(a - b).max() / np.abs(b).max():.3e}")
    gs.close()


if __name__ == "__main__":
    main()
