"""``tests/recip_cases.py`` checked on the CPU, so that ``tests/test_gpu_recip_shapes.py`` cannot pass vacuously: the longdouble
reference against mpmath at 50 digits and against the literal oracle, and -- through the host-only ``ceg_recip_launch_shape`` --
the case table against the variant each row is meant to launch (a drifted table would test one variant twice), the placements
per wave of the large batches, and the refusals."""
import numpy as np
import pytest

import ceg_hip as ceg
from ceg_hip import _abi
from ceg_hip.hostmirror.ewald import ewald_context_constants

import recip_cases as RC


def test_reference_against_mpmath():
    """40 k-vectors at most, 6 placements of a 3-atom molecule, one of them with an atom at the fractional coordinate 1/2 exactly
    (both rint calls of the reference see a tie there); mpmath evaluates exp(2 pi i k.f) at 50 digits without any reduction.
    Agreement to 2^-60 of T, the sum of the absolute values of the terms."""
    import mpmath as mp
    k = RC.kset((3, 2, 2), 1.0, seed=3)
    assert 20 <= k.nk <= 40
    inv = RC.general_cell().copy()
    inv[0] = (1.0 / 32.0, 0.0, 0.0)                              # f_x = x / 32 exactly
    q, model = RC.molecule(3, 1)
    pos = RC.placements(model, 6, 1, spread=14.0)
    pos[2, 1] = (16.0, 3.0, -2.0)                                # f_x = 0.5
    pos[3, 0] = (-16.0, 1.0, 5.0)                                # f_x = -0.5
    enc, static = -3.25, 11.5
    got = RC.reference(inv, k.ijk, k.kf, k.sf, q, pos, enc, static)
    f = pos @ inv.T
    assert f[2, 1, 0] == 0.5 and f[3, 0, 0] == -0.5
    T = RC.magnitude(k.kf, k.sf, q, enc, static)
    with mp.workdps(50):
        tp = 2 * mp.pi
        M = [[mp.mpf(float(inv[a, c])) for c in range(3)] for a in range(3)]
        for p in range(len(pos)):
            cross = own = mp.mpf(0)
            fr = [[sum(M[ax][c] * mp.mpf(float(pos[p, a, c])) for c in range(3)) for ax in range(3)] for a in range(3)]
            for v in range(k.nk):
                S = mp.mpc(0)
                for a in range(3):
                    S += mp.mpf(float(q[a])) * mp.expj(tp * sum(int(k.ijk[v, ax]) * fr[a][ax] for ax in range(3)))
                sf = mp.mpc(float(k.sf[v].real), float(k.sf[v].imag))
                cross += mp.mpf(float(k.kf[v])) * (mp.conj(sf) * S).real
                own += mp.mpf(float(k.kf[v])) * (S.real ** 2 + S.imag ** 2)
            exact = 2 * (cross + mp.mpf(enc)) + (own + mp.mpf(static))
            # the longdouble goes to mpmath through its exact high and low float64 parts
            hi = float(got[p]); lo = float(got[p] - RC.LD(hi))
            err = abs(mp.mpf(hi) + mp.mpf(lo) - exact)
            assert err <= mp.mpf(2) ** -60 * T, (p, float(err / T))


def test_reference_against_the_oracle(oracle):
    """CHA fixture, CO2, 256 placements: the project's tolerance for the reciprocal term."""
    fw = ceg.load_framework_RASPA("CHA_1.4_3b4eeb96", "BoulfelfelSholl2021")
    ef = ceg.initialize_ewald(fw, (1, 1, 1))
    co2 = ceg.load_molecule_RASPA("CO2", "TraPPE", "BoulfelfelSholl2021")
    base = np.asarray(co2.position, dtype=np.float64).reshape(-1, 3)
    pos = np.random.default_rng(4).uniform(-40, 60, (256, 1, 3)) + base[None]
    enc, static = ewald_context_constants(ef, ((co2,),))
    q = np.asarray(co2.atomic_charge, dtype=np.float64)
    got = RC.reference(ef.invmat, ef.kvec_ijk, ef.kfactors, np.asarray(ef.StoreRigidChargeFramework), q, pos, enc, static).astype(np.float64)
    ref = oracle.reciprocal_energies(ef, co2, pos)
    assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref) + 1e-11 * np.abs(ref).max())
    # and the oracle sits far inside the derived bound (its table recurrences included)
    tol = RC.bound(ef.invmat, ef.kspace.ks, ef.kfactors, np.asarray(ef.StoreRigidChargeFramework), q, pos, enc, static)
    assert np.all(np.abs(ref - got) <= tol)


def test_kset_generator():
    full = RC.kset((5, 4, 3), seed=1)
    t = {tuple(v) for v in full.ijk}
    assert len(t) == full.nk and (0, 0, 0) not in t
    assert all((-i, -j, -k) not in t for i, j, k in t)                       # a half space
    assert (5, 0, 0) in t and (0, 4, 0) in t and (0, 0, 3) in t and (0, 0, -3) not in t and (5, 1, 0) not in t
    assert np.all(full.kf > 0) and full.kf.max() / full.kf.min() > 300 and 0.03 < np.mean(full.sf == 0) < 0.2
    flat = RC.kset((0, 5, 5), seed=1)
    assert flat.nk > 20 and np.all(flat.ijk[:, 0] == 0)
    h = RC.kset((5, 4, 3), holes=7, dups=5, shuffle=True, seed=2)
    assert h.nk == full.nk - 7 + 5 and len({tuple(v) for v in h.ijk}) == full.nk - 7
    # a hole splits its row and a repeated k-vector starts a run of its own: more segments than the full set has
    assert RC.layout(h)[2] > RC.layout(full)[2]
    for nseg in (64, 65, 128, 129):
        t = RC.trimmed_to_segments(RC.kset(RC.SEGMENT_KS, seed=6), nseg)
        nr, _ns, got = RC.layout(t)
        assert got == nseg and nr == (nseg + 63) // 64


@pytest.mark.parametrize("name", sorted(RC.VARIANTS))
def test_variant_table_selects_every_instantiation(name):
    ks, _rho, natoms, (c_in_lds, waves) = RC.VARIANTS[name]
    k = RC.variant_kset(name)
    w, c, pw, lds = RC.launch_shape(k, natoms, RC.N_RAGGED)
    assert (c, w, pw) == (c_in_lds, waves, 1), (name, w, c, pw)
    assert RC.N_RAGGED % waves != 0 or waves == 1                             # ragged last workgroup
    assert lds <= 65536 and lds + RC.LDS_STATIC <= 160 * 1024
    nr, ns, _nseg = RC.layout(k)
    c_bytes = 8 * 3 * ns * 64 + 4 * ((nr * 64 + 3) & ~3)
    assert lds == 16 * waves * natoms * k.stride + (c_bytes if c_in_lds else 0)
    chunk = RC.per_wave_one_chunk(waves)
    assert RC.launch_shape(k, natoms, chunk)[2] == 1 and (chunk % waves != 0 or waves == 1)
    for pw in (2, 4, 8):
        n = RC.big_n(pw, waves)
        got = RC.launch_shape(k, natoms, n)
        assert got[:3] == (waves, c_in_lds, pw if c_in_lds else 1), (name, pw, got)
        # the last workgroup: r placements over waves of pw each -- one partial range, and with several waves an empty one
        r = n % (pw * waves)
        ranges = [max(0, min(pw, r - wv * pw)) for wv in range(waves)]
        assert any(0 < x < pw for x in ranges) and (waves == 1 or 0 in ranges)
        assert RC.launch_shape(k, natoms, n - r - 1)[2] == pw // 2 or not c_in_lds       # n is just past the threshold


def test_variant_table_is_complete():
    assert {v[3] for v in RC.VARIANTS.values()} == {(c, w) for c in (True, False) for w in (8, 4, 2, 1)}
    seen = set()
    for name, (_ks, _rho, natoms, (c, w)) in RC.VARIANTS.items():
        if c:
            k = RC.variant_kset(name)
            seen |= {(w, RC.launch_shape(k, natoms, n)[2]) for n in [RC.N_RAGGED] + [RC.big_n(pw, w) for pw in (2, 4, 8)]}
    assert seen == {(w, pw) for w in (8, 4, 2, 1) for pw in (1, 2, 4, 8)}


def test_launch_shape_refusals():
    lib = _abi.load_library()
    k = RC.kset((3, 3, 3), seed=1)
    out = np.zeros(4, dtype=np.int32)

    def rc(kk, natoms, n, ijk="own"):
        p = (_abi.i32ptr(np.ascontiguousarray(kk.ijk.reshape(-1))) if kk.nk else None) if ijk == "own" else ijk
        return lib.ceg_recip_launch_shape(p, kk.nk, _abi.i32ptr(kk.ks), natoms, n, _abi.i32ptr(out))

    assert rc(k, 16, 100) == 0
    assert rc(k, 17, 100) == -5 and b"16" in lib.ceg_last_error()
    assert rc(k, 0, 100) == -1 and rc(k, 1, -1) == -1 and rc(k, 1, 100, ijk=None) == -1
    assert rc(k, 1, 0) == 0 and out[2] == 1
    # the box: stride 400 is the largest, 401 is refused like ceg_recip_create refuses it
    assert rc(RC.with_constants((133, 66, 66), [[1, 0, 0]], 1), 1, 10) == 0
    assert rc(RC.with_constants((134, 66, 66), [[1, 0, 0]], 1), 1, 10) == -5 and b"k-space box" in lib.ceg_last_error()
    assert rc(RC.with_constants((-1, 2, 2), [[0, 0, 1]], 1), 1, 10) == -5
    # a k-vector outside the box
    assert rc(RC.with_constants((3, 3, 3), [[4, 0, 0]], 1), 1, 10) == -1 and b"k-vector" in lib.ceg_last_error()
    assert rc(RC.with_constants((3, 3, 3), [[1, -4, 0]], 1), 1, 10) == -1
    # one wave's tables above 64 KiB: natoms x stride > 4096
    big = RC.with_constants((133, 66, 66), [[1, 0, 0]], 1)
    assert rc(big, 10, 10) == 0 and out[0] == 1 and out[3] == 64000
    assert rc(big, 11, 10) == -5 and b"LDS" in lib.ceg_last_error()
    edge = RC.with_constants((101, 38, 38), [[1, 0, 0]], 1)                   # stride 102 + 77 + 77 = 256
    assert edge.stride == 256 and rc(edge, 16, 10) == 0 and out[0] == 1 and out[3] >= 65536
    edge = RC.with_constants((102, 38, 38), [[1, 0, 0]], 1)                   # stride 257: 16 x 257 > 4096
    assert rc(edge, 16, 10) == -5
    # no placements and no k-vectors are no refusal
    assert rc(RC.with_constants((0, 0, 0), np.empty((0, 3)), 1), 1, 5) == 0 and tuple(out) == (8, 1, 1, 16 * 8 * 3)


def test_edge_cases_are_what_their_names_say():
    e = RC.edge_ksets()
    assert e["nk0-box0"].nk == 0 and e["nk0-box3"].nk == 0 and e["nk1"].nk == 1
    for name, ax in (("kx0", 0), ("ky0", 1), ("kz0", 2)):
        assert e[name].ks[ax] == 0 and np.all(e[name].ijk[:, ax] == 0) and e[name].nk > 20
    assert tuple(e["line"].ks) == (6, 0, 0) and e["line"].nk == 6
    assert RC.layout(e["row21"])[0] == 1 and np.array_equal(np.sort(e["row21"].ijk[:, 0]), np.arange(21))      # one row cut into segments of one round
    for nseg in (64, 65, 128, 129):
        assert RC.layout(e[f"seg{nseg}"])[2] == nseg
    h = e["holes-dups-shuffled"]
    assert len({tuple(v) for v in h.ijk}) == h.nk - 9 and not np.array_equal(h.ijk, h.ijk[np.lexsort((h.ijk[:, 0], h.ijk[:, 2], h.ijk[:, 1]))])
    b = RC.box400()
    t = {tuple(v) for v in b.ijk}
    assert b.stride == 400 and {(i, 1, 0) for i in range(134)} <= t and {(133, j, k) for j in (-66, 66) for k in (-66, 66)} <= t
    assert RC.launch_shape(b, 1, 130)[0] == 4 and RC.launch_shape(b, 4, 130)[0] == 1
    assert RC.launch_shape(e["tab-64k"], 16, 130) == (1, False, 1, 65536)
    for natoms in (2, 5):
        w, c, pw, lds = RC.launch_shape(RC.window_kset(natoms), natoms, 130)
        assert c and pw == 1 and 65536 - RC.LDS_STATIC < lds <= 65536
