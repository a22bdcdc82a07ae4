"""``ceg_grid_basins`` / ``ceg_hip.basins.local_basins`` against the literal, queue-based restatements of ``tests/basin_flow_cases.py``
(the host NumPy form for the two 300 k-point cases, which ``test_basin_flow_host.py`` ties to the literal on the smaller shapes).
Every integer is compared with ``==``: level, owner, nowners, shared, size.  Every case runs once from host arrays through the binding
and once from device arrays (torch tensors) with device outputs through the C ABI.  The references are computed once per case."""
import ctypes as C
import math

import numpy as np
import pytest

import basin_flow_cases as FC
import basins_cases as BC
from ceg_hip import _abi, basins as B

pytestmark = pytest.mark.gpu

NULL = C.c_void_p(0)
CASES = FC.basin_cases()
FIELDS = ("level", "owner", "nowners", "shared", "size")


def _ids(cases):
    return [c[0] for c in cases]


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(arr).ravel(order="F"))).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _dims(d):
    return _abi.i32ptr(np.asarray(d, dtype=np.int32))


def _device_call(hip_lib, g, starts, kw, shared_cap, stream=NULL, dstarts=None):
    """device grid, device starts, device outputs filled with -7 beforehand -> (rc, dict of host copies, count)"""
    import torch
    n, ns = g.size, len(starts)
    dg = _dev(g)
    if dstarts is None:
        dstarts = torch.from_numpy(np.asarray(starts, dtype=np.int32).reshape(-1, 3)).cuda()
    dlevel = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    downer = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dnown = torch.full((n,), 249, dtype=torch.uint8, device="cuda")
    dshared = torch.full((shared_cap + 1, 2), -7, dtype=torch.int32, device="cuda")
    dsize = torch.full((ns + 1,), -7, dtype=torch.int32, device="cuda")
    count = C.c_int64(-1)
    torch.cuda.synchronize()
    rc = hip_lib.ceg_grid_basins(0, _ptr(dg), 1, _dims(g.shape), _ptr(dstarts), 1, ns, int(kw.get("maxima", False)),
                                 float(kw.get("skip_above", math.inf)), int(kw.get("maxdist", 0)), _ptr(dlevel), _ptr(downer), _ptr(dnown), 1,
                                 _ptr(dshared), shared_cap, C.byref(count), _ptr(dsize), 1, stream)
    torch.cuda.synchronize()
    out = dict(level=dlevel.cpu().numpy().reshape(g.shape, order="F"), owner=downer.cpu().numpy().reshape(g.shape, order="F"),
               nowners=dnown.cpu().numpy().reshape(g.shape, order="F"), shared=dshared.cpu().numpy(), size=dsize.cpu().numpy())
    return rc, out, count.value


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_basins_from_host_arrays(hip_lib, case):
    name, g, starts, kw, _ = case
    want = FC.expected(name)
    b = B.local_basins(g, starts, **kw)
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), want[f]), f
    assert b.kept.tolist() == np.flatnonzero(want["size"] > 0).tolist()


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_basins_from_device_arrays_and_the_shared_capacity(hip_lib, case):
    """room for half of the pairs: the full count, the head of the list, nothing past the end; sizes and maps complete"""
    name, g, starts, kw, _ = case
    want = FC.expected(name)
    total = len(want["shared"])
    cap = total // 2
    rc, got, count = _device_call(hip_lib, g, starts, kw, cap)
    assert rc == 0, hip_lib.ceg_last_error()
    assert count == total
    for f in ("level", "owner", "nowners"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["size"][:len(starts)], want["size"]) and got["size"][len(starts)] == -7
    assert np.array_equal(got["shared"][:cap], want["shared"][:cap])
    assert (got["shared"][cap:] == -7).all()


def test_shared_with_room_to_spare_and_without_any(hip_lib):
    name, g, starts, kw, _ = FC.case("smooth-17x9x33")
    want = FC.expected(name)
    total = len(want["shared"])
    assert total > 2
    rc, got, count = _device_call(hip_lib, g, starts, kw, total + 5)
    assert rc == 0 and count == total
    assert np.array_equal(got["shared"][:total], want["shared"]) and (got["shared"][total:] == -7).all()
    # no room and no outputs at all but the count
    count = C.c_int64(-1)
    dg = _dev(g)
    st = np.asarray(starts, dtype=np.int32)
    _abi.check(hip_lib, hip_lib.ceg_grid_basins(0, _ptr(dg), 1, _dims(g.shape), C.c_void_p(st.ctypes.data), 0, len(st), 0, math.inf, 0, NULL, NULL,
                                                NULL, 0, NULL, 0, C.byref(count), NULL, 0, NULL))
    assert count.value == total


def test_more_starts_than_the_size_table_in_lds_and_the_owner_map_alone(hip_lib):
    """up to 8192 starts the sizes are counted in an LDS table per workgroup first, beyond that (and when only the owner map is asked
    for) the runs go to global memory directly: a random 70 x 66 x 65 field has more minima than that"""
    import torch
    g = BC._rng(41, 70, 66, 65).uniform(-3.0, 1.0, size=(70, 66, 65))
    starts = B.local_minima_host(g, -1.0)
    assert len(starts) > 8192
    want = B.local_basins_host(g, starts)
    b = B.local_basins(g, starts)
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), getattr(want, f)), f
    dg = _dev(g)
    downer = torch.full((g.size,), -7, dtype=torch.int32, device="cuda")
    few = np.ascontiguousarray(starts[:50])
    torch.cuda.synchronize()
    _abi.check(hip_lib, hip_lib.ceg_grid_basins(0, _ptr(dg), 1, _dims(g.shape), C.c_void_p(few.ctypes.data), 0, len(few), 0, math.inf, 0, NULL,
                                                _ptr(downer), NULL, 1, NULL, 0, None, NULL, 0, NULL))
    torch.cuda.synchronize()
    assert np.array_equal(downer.cpu().numpy().reshape(g.shape, order="F"), B.local_basins_host(g, few).owner)


def test_on_a_stream_and_of_a_c_ordered_input(hip_lib):
    import torch
    name, g, starts, kw, _ = FC.case("smooth-17x9x33-skip")
    want = FC.expected(name)
    st = torch.cuda.Stream()
    gc = np.ascontiguousarray(g)
    assert gc.flags.c_contiguous and not gc.flags.f_contiguous
    b = B.local_basins(gc, starts, stream=st.cuda_stream, **kw)                     # C-ordered input: the binding reorders it
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), want[f]), f
    rc, got, count = _device_call(hip_lib, g, starts, kw, len(want["shared"]), stream=C.c_void_p(st.cuda_stream))
    assert rc == 0 and count == len(want["shared"])
    for f in ("level", "owner", "nowners"):
        assert np.array_equal(got[f], want[f]), f
    dg = _dev(g)
    b = B.local_basins((dg.data_ptr(), g.shape), starts, stream=st.cuda_stream, **kw)
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), want[f]), f


def test_a_short_owner_pool_runs_the_owner_pass_again(hip_lib, monkeypatch):
    """the pool of owner lists starts at max(a*b*c, 4096) entries; with a first size of 8 entries the pass is repeated with the bound"""
    name, g, starts, kw, _ = FC.case("smooth-17x9x33")
    want = FC.expected(name)
    assert len(want["shared"]) > 8
    monkeypatch.setenv("CEG_HIP_BASINS_POOL", "8")
    b = B.local_basins(g, starts, **kw)
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), want[f]), f
    fg, fst = FC.fan(4)
    assert np.array_equal(B.local_basins(fg, fst).shared, FC.expected("fan-16")["shared"])


def test_refusals(hip_lib):
    _, g, starts, kw, _ = FC.case("random-5x7x3")
    assert len(starts) >= 2
    with pytest.raises(_abi.CegError) as err:
        B.local_basins(g, list(starts) + [starts[1]])
    assert err.value.code == -1 and f"start {len(starts)} repeats" in str(err.value)
    for bad in ((5, 0, 0), (0, -1, 0), (0, 0, 3)):
        with pytest.raises(_abi.CegError) as err:
            B.local_basins(g, list(starts) + [bad])
        assert err.value.code == -1 and f"start {len(starts)} is outside" in str(err.value)
    rc, _, _ = _device_call(hip_lib, g, list(starts) + [starts[0]], {}, 4)             # the same from a device list
    assert rc == -1 and b"repeats" in hip_lib.ceg_last_error()
    with pytest.raises(_abi.CegError) as err:
        B.local_basins(g, starts, skip_above=math.nan)
    assert err.value.code == -1
    assert B.local_basins(g, starts).size.sum() > 0                                  # a valid call follows


def test_the_fan_at_the_cap_and_above_it(hip_lib):
    """R = 4: 16 starts own the centre, exactly CEG_BASINS_MAX_OWNERS, legal.  R = 5: 20 owners, refused with the index and the count."""
    g, starts = FC.fan(4)
    b = B.local_basins(g, starts)
    assert b.nowners[5, 5, 0] == 16 == _abi.BASINS_MAX_OWNERS and b.nowners.max() == 16
    centre = 5 + 11 * 5
    assert b.shared[b.shared[:, 0] == centre, 1].tolist() == list(range(16))
    g, starts = FC.fan(5)
    assert len(starts) == 20
    with pytest.raises(_abi.CegError) as err:
        B.local_basins(g, starts)
    assert err.value.code == -5                                                      # CEG_ERR_UNSUPPORTED
    assert f"grid point {centre} has 20 owners" in str(err.value)
    rc, _, _ = _device_call(hip_lib, g, starts, {}, 64)
    assert rc == -5 and b"has 20 owners" in hip_lib.ceg_last_error()
    host = B.local_basins_host(g, starts)                                            # the host form has no cap
    assert host.nowners[5, 5, 0] == 20


def test_device_chaining_from_the_minima_list(hip_lib):
    """ceg_grid_local_minima with a device list, then ceg_grid_basins reading that list on the device; and the binding's own route"""
    import torch
    name, g, tol, maxima = next(c for c in BC.minima_cases() if c[0] == "wrap-17x9x33-tol-1.0")
    ref, _ = BC.minima_reference(name)
    want = FC.expected("wrap-17x9x33")
    dg = _dev(g)
    dijk = torch.full((len(ref) + 3, 3), -7, dtype=torch.int32, device="cuda")
    count = C.c_int64(-1)
    torch.cuda.synchronize()
    _abi.check(hip_lib, hip_lib.ceg_grid_local_minima(0, _ptr(dg), 1, _dims(g.shape), 0, tol, _ptr(dijk), 1, len(ref) + 3, C.byref(count), None,
                                                      NULL))
    assert count.value == len(ref)
    rc, got, cnt = _device_call(hip_lib, g, ref, {}, len(want["shared"]), dstarts=dijk)
    assert rc == 0 and cnt == len(want["shared"])
    for f in ("level", "owner", "nowners"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["shared"][:cnt], want["shared"]) and np.array_equal(got["size"][:len(ref)], want["size"])
    b = B.local_basins(g)                                                            # minima=None: local_minima first, the list stays on the device
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), want[f]), f
    b = B.local_basins((dg.data_ptr(), g.shape))
    assert np.array_equal(b.owner, want["owner"])


@pytest.mark.parametrize("cluster", [1, 3])
def test_cluster_and_decompose_through_the_device(hip_lib, cluster):
    name = "random-17x9x33"
    _, g, starts, kw, _ = FC.case(name)
    ref = FC.literal_reference(name, cluster=cluster)
    b = B.local_basins(g, starts, cluster=cluster)
    assert b.kept.tolist() == ref["kept"]
    assert [set(map(tuple, B.basin_points(b, int(i)).tolist())) for i in b.kept] == ref["basins"]
    points, nodes = FC.decompose_basins_literal(g.shape, ref["basins"])
    got_points, offsets, owners = B.decompose_basins(b)
    assert [tuple(p) for p in got_points.tolist()] == points
    assert all(tuple(owners[offsets[n]:offsets[n + 1]].tolist()) == nodes[p] for n, p in enumerate(points))
    h = B.local_basins_host(g, starts, cluster=cluster)
    for f in FIELDS:
        assert np.array_equal(getattr(b, f), getattr(h, f)), f
