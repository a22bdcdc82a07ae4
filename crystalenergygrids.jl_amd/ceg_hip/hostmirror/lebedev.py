"""Orientations of a rigid molecule (mirror of ``src/lebedev.jl:4`` and ``:109-123``).

The reference reads its Lebedev points from an artifact it downloads (``Artifacts.toml``); no table is shipped here, so the
unit vectors are an argument.  What is restated is what the reference does WITH the points: ``read_lebedev_grid`` turns every
point by the fixed matrix ``_rotmatrix`` (lebedev.jl:29), ``get_rotation_matrices`` builds one matrix per (z-rotation, point)
(lebedev.jl:117-122)."""
from __future__ import annotations

import math

import numpy as np

# lebedev.jl:4
_rotmatrix = np.array([[-0.17963068200890037, -0.21953827352603253, -0.9589242746631385],
                       [-0.9599246581752935, 0.25228151379218244, 0.12206018362173197],
                       [0.21512198564550156, 0.9424208106021077, -0.2560577025515984]])


def _sinpi(x: float) -> float:
    """Julia's sinpi: exact at the multiples of 1/2 (sinpi(2i/5) has no such argument, the reduction keeps the angle small)."""
    x = math.fmod(x, 2.0)
    return math.sin(math.pi * x) if x <= 1.0 else -math.sin(math.pi * (2.0 - x))


def _cospi(x: float) -> float:
    x = math.fmod(x, 2.0)
    return math.cos(math.pi * x) if x <= 1.0 else math.cos(math.pi * (2.0 - x))


def rotation_matrices(points, islinear: bool) -> np.ndarray:
    """lebedev.jl:117-122 for caller-supplied unit vectors ``points[n, 3]`` (raw Lebedev points, before ``_rotmatrix``):

        zrots = [[cospi(2i/5) -sinpi(2i/5) 0; sinpi(2i/5) cospi(2i/5) 0; 0 0 1] for i in 0:(4-4islin)]          (:117)
        for zrot in zrots, point in lebedev.points:  rots <- hcat([1, 0, 0], [0, 1, 0], point) * zrot            (:119-121)

    with ``lebedev.points[i] = _rotmatrix * p[i]`` (:29).  -> float64[(1 or 5) * n, 3, 3], z-rotation outermost.  As in the
    reference the matrices are NOT orthogonal (the first two columns are e1 and e2 turned about z, the third is the point).
    The halving of the points of a linear symmetric molecule (:30-41) and the weights are the caller's."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pts = pts @ _rotmatrix.T                                          # :29
    rots = []
    for i in range(0, (4 - 4 * bool(islinear)) + 1):                  # :117
        c, s = _cospi(2 * i / 5), _sinpi(2 * i / 5)
        zrot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        for point in pts:                                             # :119 (zrot outer, point inner)
            h = np.array([[1.0, 0.0, point[0]], [0.0, 1.0, point[1]], [0.0, 0.0, point[2]]])       # hcat(e1, e2, point), :120
            rots.append(h @ zrot)
    return np.array(rots, dtype=np.float64).reshape(-1, 3, 3)
