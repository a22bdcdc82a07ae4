"""The sequential part of the site extraction without a device: the nearest-basin rule that ``ceg_grid_coalesce`` follows against the literal
loop of ``tests/site_extraction_cases.py`` bit for bit, ``ceg_cluster_closer_than`` (host code of the library) against its literal, the two
under the sanitizers as a stand-alone program, and the conditions on the INPUTS that ``tests/test_gpu_site_coalesce.py`` relies on: the
number of basins a case reaches, the voxels that hit a basin changed earlier in their batch, the search branch of the distance, exact ties,
and that the order of additions shows in the bits."""
import ctypes as C
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import site_coalesce_cases as CC
import site_extraction_cases as SC
from ceg_hip import _abi, basins as B

ROOT = Path(__file__).resolve().parent.parent


def _ids(cases):
    return [c[0] for c in cases]


def _same(got, ref):
    """two lists of (value, centre): the same bits"""
    assert len(got) == len(ref)
    for (v, p), (rv, rp) in zip(got, ref):
        assert np.array_equal(np.asarray([v, *p], dtype=np.float64).view(np.int64), np.asarray([rv, *rp], dtype=np.float64).view(np.int64))


def _host_pass(case):
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    return B.coalesce_ranked(lin, sm, CC.values_of(grid, counter)[lin], dims, mat, maxdist, atol, maxbasins)


SMALL = [c for c, _ in CC.small_cases()]


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("case,want", CC.small_cases(), ids=_ids(SMALL))
def test_nearest_rule_is_the_literal_loop(case, want):
    """the rule the device follows gives the bits of :677-719 as written, and so does the library's host pass; the statistics the
    case was built for hold"""
    name, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    ref, br = CC.expected_small(name)
    assert br["maxsubmid"] <= 1 and br["merge"] == 0                              # the collapse of :695-699 the rule rests on
    ret, st = CC.nearest_rule(lin, sm, CC.values_of(grid, counter), dims, mat, maxdist, atol, maxbasins)
    _same(ret, ref)
    _same(_host_pass(case), ref)
    assert st["founders"] == br["new"] and st["lone"] == br["lone_low"] and st["absorbed"] == br["absorb"]
    for key, n in want.items():
        if key in ("moved", "dirty", "rescans"):
            assert st[key] >= n, (key, st)
        else:
            assert st[key] == n, (key, st)
    print(name, st)


@pytest.mark.parametrize("case", CC.length_cases(), ids=_ids(CC.length_cases()))
def test_lengths_around_the_batch(case):
    ref, _ = CC.expected_small(case[0])
    _same(_host_pass(case), ref)
    assert len(ref) >= min(len(case[1]), 1)


def test_lone_push_is_not_pos():
    """(val, pos*val/val) differs from (val, pos) in the cases that check it, and the lone push does not end the loop"""
    for cname in ("ortho", "skew"):
        ref, br = CC.expected_small(f"lone-low-bits-{cname}")
        val, cen = ref[1]
        pos = [9 / 12, 4 / 10, 8 / 14]
        assert br["lone_low"] == 1 and val == 0.09 and list(cen) == [p * val / val for p in pos]
        assert cen[0] != pos[0] and cen[1] != pos[1]
    case = next(c for c in SMALL if c[0] == "value-branches")
    ref, br = CC.expected_small("value-branches")
    assert br["lone_low"] == 1 and br["maxbasins"] == 1 and br["zero"] == 2 and br["new"] == 3
    assert len(ref) == 4 > case[9] and len(case[1]) == 9                          # three basins did not stop it; two voxels are never reached


@pytest.mark.parametrize("name", ["one-basin-takes-a-batch", "drift", "skew-scattered", "cit7-scattered"])
def test_the_order_of_the_ranking_shows_in_the_bits(name):
    case = next(c for c in SMALL if c[0] == name)
    _, lin, sm, grid, counter, dims, mat, maxdist, atol, maxbasins = case
    values = CC.values_of(grid, counter)
    ref, _ = CC.nearest_rule(lin, sm, values, dims, mat, maxdist, atol, maxbasins)
    other, _ = CC.nearest_rule(np.concatenate([lin[:1], lin[:0:-1]]), sm, values, dims, mat, maxdist, atol, maxbasins)
    bits = lambda ret: [np.asarray([v, *p]).view(np.int64).tolist() for v, p in ret]      # noqa: E731
    assert bits(ref) != bits(other)


@pytest.mark.parametrize("nf", CC.FOUNDER_COUNTS)
def test_founder_cases_reach_their_count(nf):
    case = CC.founder_case(nf)
    ret = _host_pass(case)
    assert len(ret) == nf and len(case[1]) == 2 * nf
    if nf <= CC.T + 1:                                                            # the rule in Python where that stays quick
        got, st = CC.nearest_rule(*case[1:3], CC.values_of(case[3], case[4]), *case[5:])
        _same(got, ret)
        assert st["founders"] == nf and st["absorbed"] == nf and st["ties"] >= 1, st
        print(nf, st)


def test_random_map_and_many_basins_inputs():
    bins, counter, dims, mat, maxdist = CC.random_map()
    values = CC.values_of(bins, counter)
    lin, smv = B.ranked_above_host(values.reshape(dims, order="F"), 0.0)
    ret = B.coalesce_ranked(lin, smv, values[lin], dims, mat, maxdist, 0.0)
    assert len(lin) > 20 * CC.T and 30 <= len(ret) < len(lin)
    bins, counter, dims, mat, maxdist, kw = CC.many_basins_case()
    values = CC.values_of(bins, counter)
    lin, smv = B.ranked_above_host(values.reshape(dims, order="F"), 0.0)
    ret = B.coalesce_ranked(lin, smv, values[lin], dims, mat, maxdist, kw["atol"])
    assert len(ret) == 13 ** 3 > _abi.SITE_PROXIMITY_MAX_SITES


# ---------------------------------------------------------------------------------------------------------------- partition
def _partition_host(grid, counter, dims, mat, sites, origin=0):
    values = CC.values_of(grid, counter)
    lin, site, off, _ = B.site_nearest_host(sites, dims, mat, bins=(values != 0).reshape(dims, order="F"), origin=origin, want_dist=False)
    return B._accumulate_closest(values, dims, len(sites), lin, site, off, []), lin, site


def test_partition_inputs():
    cases = {c[0]: c for c in CC.partition_cases()}
    # the cap: the second and the fourth voxel of the row are skipped, the third and the fifth are accepted
    _, grid, counter, dims, mat, sites = cases["ortho-cap"]
    ref, lin, site = _partition_host(grid, counter, dims, mat, sites)
    assert ref.cap_bound and site.tolist() == [0, 0, 0, 0, 0, 1]
    assert ref.sums[0] == (0.6 + 0.3) + 0.1 and ref.sums[0] <= 1 and ref.sums[1] == 0.25
    # an empty site, a site with one voxel, and generic values: another order of the additions gives other bits
    _, grid, counter, dims, mat, sites = cases["skew-generic-empty-and-single"]
    ref, lin, site = _partition_host(grid, counter, dims, mat, sites)
    counts = np.bincount(site, minlength=3)
    assert counts.tolist() == [64, 1, 0] and not ref.cap_bound and np.all(np.isnan(ref.centres[2])) and ref.sums[2] == 0
    vals = CC.values_of(grid, counter)[lin[site == 0]]
    fwd, back = 0.0, 0.0
    for v in vals.tolist():
        fwd += v
    for v in vals.tolist()[::-1]:
        back += v
    assert fwd == ref.sums[0] and back != fwd
    one, _, site = _partition_host(*cases["skew-generic-one-site"][1:])
    assert len(site) == 65 and not site.any()
    # more sites than voxels: most sites stay empty, and the search branch and the site limit are crossed
    for ns in (2047, 2048, 2049, 4097):
        _, grid, counter, dims, mat, sites = cases[f"cit7-70x66x65-{ns}"]
        assert len(sites) == ns and 20 <= np.count_nonzero(grid) <= 45


# ---------------------------------------------------------------------------------------------------------------- cluster_closer_than
@pytest.mark.parametrize("case", CC.cluster_cases(), ids=_ids(CC.cluster_cases()))
def test_cluster_closer_than_in_the_library(case):
    name, ret, mat, maxdist = case
    ref = SC.cluster_closer_than_literal(ret, mat, maxdist)
    _same(B.cluster_closer_than(ret, mat, maxdist), ref)
    _same(B.cluster_closer_than_host(ret, mat, maxdist), ref)
    kind = name.split("-")[1]
    if kind == "cap":
        assert len(ref) == 2 and ref[0][0] == 0.6 + 0.3                           # 0.6 + 0.5 > 1: left apart, before any distance
    elif kind == "chain":
        assert len(ref) == 1
    elif kind == "wrap":
        assert len(ref) == 1 and ref[0][0] == (0.2 + 0.3) + 0.1
    elif kind == "300":
        assert 10 < len(ref) < 300
    else:
        assert len(ref) == min(int(kind), 1)


def test_cluster_closer_than_refusals():
    lib = _abi.load_library()
    m = np.ascontiguousarray(SC.ORTHO_MAT.T).ravel()
    rho, pos, count = np.ones(2), np.zeros(6), C.c_int64(0)
    assert lib.ceg_cluster_closer_than(_abi.dptr(rho), _abi.dptr(pos), -1, _abi.dptr(m), 1, 5.0, 1.0, C.byref(count)) == -1
    assert lib.ceg_cluster_closer_than(_abi.dptr(rho), _abi.dptr(pos), 2, _abi.dptr(m), 1, 5.0, math.nan, C.byref(count)) == -1
    assert lib.ceg_cluster_closer_than(None, None, 0, _abi.dptr(m), 1, 5.0, 1.0, C.byref(count)) == 0 and count.value == 0


def test_cluster_and_rule_under_the_sanitizers(tmp_path):
    """``csrc/ceg_coalesce.h`` with the stand-alone ``tests/native/cluster_sanitize.cpp`` under -fsanitize=address,undefined"""
    cxx = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "cluster_sanitize"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-I", str(ROOT / "crystalenergygrids.jl_amd" / "csrc"), str(ROOT / "tests" / "native" / "cluster_sanitize.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "cluster ok" in out.stdout and "DIFFERENT" not in out.stdout
