"""``ceg_site_tables`` / ``ceg_site_tables_device`` (k_site_points, k_site_recip_pairs, k_site_real_pairs of csrc/ceg_site.hip) on the
cases of ``tests/site_table_cases.py``: every compared element against the longdouble reference within the tolerance derived there,
blocked sites and hard-sphere overlaps not below 1e90, the diagonal 1e100, [i][j] and [j][i] the same bytes, the host-array and the
device-array entry point the same bytes.  ``tests/test_site_table_cases_host.py`` checks the cases, the reference and the bounds on
the CPU.  Every input is generated from seeds in the case module.

Measured on an MI355X: the 36 tests of the module take 1.6 s together, references included (the slowest, 0.19 s, is the first one: it
builds the grids); no test runs a subprocess or changes the environment.  Worst error / tolerance per case family: the docstring of the
case module and DESIGN.md (the paragraph on the site tables' reference)."""
import numpy as np
import pytest

import site_table_cases as S

pytestmark = pytest.mark.gpu
RATIOS = {}


def _run(name, hip_lib):
    c = S.BY_NAME[name]
    dev = S.Device(c, hip_lib)
    try:
        pos = S.sites(name)
        fw, rec, it, rc = dev.tables(pos)
        assert rc == 0, (name, rc, hip_lib.ceg_last_error())
        dfw, drec, dit, drc = dev.tables_device(pos)
        assert drc == 0, (name, drc, hip_lib.ceg_last_error())
        assert dfw.tobytes() == fw.tobytes() and drec.tobytes() == rec.tobytes() and dit.tobytes() == it.tobytes(), (name, "host and device entry points differ")
        return dev, pos, fw, rec, it
    except BaseException:
        dev.close()
        raise


@pytest.mark.parametrize("name", S.COMPARED)
def test_tables_against_the_longdouble_reference(hip_lib, name):
    c = S.BY_NAME[name]
    e = S.expected(name)
    dev, pos, fw, rec, it = _run(name, hip_lib)
    try:
        ratios = S.compare(e, fw, rec, it)
        RATIOS[name] = ratios
        print(f"{name}: worst error / bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
        if c.k.nk == 0 or c.charges == "zero":
            # no contraction, or one of exact zeros: recip is the offset bit for bit and the pair entries are (P + 0) + offset_pair
            assert (rec == S.OFFSET_ONE).all()
            soft = ~e.hard
            err = np.abs(it[e.I, e.J][soft].astype(S.LD) - (e.P[soft] + S.LD(S.OFFSET_PAIR)))
            assert (err <= S.LD(1e-9) * e.P_size[soft] + 4.0 * S.U * (e.P_size[soft] + abs(S.OFFSET_PAIR))).all()
        if c.table == "empty":
            assert not e.hard.any() and (np.abs(it[e.I, e.J].astype(S.LD) - (e.R + S.LD(S.OFFSET_PAIR))) <= e.R_tol + 4.0 * S.U * (S.pair_magnitude(c) + abs(S.OFFSET_PAIR))).all()
        if name == "edges-n33":
            # recip = NULL: the other two outputs are the same bytes
            fw2, none, it2, rc = dev.tables(pos, with_recip=False)
            assert rc == 0 and none is None and fw2.tobytes() == fw.tobytes() and it2.tobytes() == it.tobytes()
    finally:
        dev.close()


def test_lds_limit_refusal_leaves_the_outputs_untouched(hip_lib):
    c = S.BY_NAME["lds-stride257"]
    assert 16 * c.m * c.k.stride > 64 * 1024
    dev = S.Device(c, hip_lib)
    try:
        pos = S.sites(c.name)
        sentinel = -12345.678
        fw, rec, it, rc = dev.tables(pos, fill=sentinel)
        assert rc == -5 and b"LDS" in hip_lib.ceg_last_error(), (rc, hip_lib.ceg_last_error())                # CEG_ERR_UNSUPPORTED
        assert (fw == sentinel).all() and (rec == sentinel).all() and (it == sentinel).all()
        dfw, drec, dit, drc = dev.tables_device(pos, fill=sentinel)
        assert drc == -5 and (dfw == sentinel).all() and (drec == sentinel).all() and (dit == sentinel).all()
    finally:
        dev.close()


def test_threshold_decisions_are_literal_r2s(hip_lib):
    """pairs at +-1e-12, +-2e-16 and 0 relative to cutoff^2 and to the hard-sphere radius^2: the table holds exactly +inf, -1.75 +
    offset_pair or offset_pair, by the r^2 that ``literal_r2`` forms"""
    c = S.BY_NAME["thresholds"]
    dev, pos, fw, rec, it = _run(c.name, hip_lib)
    try:
        want = S.threshold_expected(c)
        bad = np.nonzero(it != want)
        assert not len(bad[0]), (list(zip(bad[0][:8].tolist(), bad[1][:8].tolist())), it[bad][:8], want[bad][:8])
        assert (rec == S.OFFSET_ONE).all() and (fw == S.OFFSET_ONE).all()
    finally:
        dev.close()
