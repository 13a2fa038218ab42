"""The leaf routines of the contact engines (d3il_amd/csrc/rigid_common.h, and the twins compiled in gen_tree.h) by themselves on the host build: box_box,
cyl_box, cone_eval / gt_cone_eval, ldl_n / gt_ldl_n with their solves, cube_integrate, push_tan_yaw and quat2mat against the stored problems and references of
tests/contact_leaf_cases.py (40-digit mpmath values, the oracle's colliders, geometric invariants).  The device build: tests/test_gpu_contact_leaf.py."""
import numpy as np
import pytest

from tests import contact_leaf_cases as K


@pytest.fixture(scope="module")
def cases():
    return K.Cases()


@pytest.mark.parametrize("swapped", (False, True))
def test_box_box(cases, swapped):
    """Stable cases: the oracle's count and contacts in order at 1e-12; tie cases: one of the oracle's answers as a set; every case: the geometric invariants.
    Both geom orders (gen_phase2 calls the routine with the static box first or second)."""
    count, rec = K.host_box(cases.box, swapped)
    bad, _ = K.check_box(cases.box, count, rec, "host", swapped=swapped)
    assert not bad, "\n".join(bad[:20])


def test_box_box_cap(cases):
    """cap < the number of contacts: the first `cap` contacts of the full answer, nothing past them."""
    g = cases.box
    full_n, full = K.host_box(g)
    for cap in (0, 1, 3):
        n, rec = K.host_box(g, cap=cap)
        assert np.array_equal(n, np.minimum(full_n, cap))
        for i in range(g.n):
            assert np.array_equal(rec[i, :n[i]], full[i, :n[i]]) and np.isnan(rec[i, n[i]:]).all()


def test_cyl_box(cases):
    hit, out = K.host_cyl(cases.cyl)
    bad = K.check_cyl(cases.cyl, hit, out, "host")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("twin", (False, True))
def test_cone_eval(cases, twin):
    """Cost, force and Hessian against the differentiated cost, 4 yardsticks; apex scales 1e-105 .. 1e-170: cost and force, the Hessian's finiteness recorded."""
    out = K.host_cone(cases.cone, twin)
    bad, worst, fin = K.check_cone(cases.cone, out, "host/gt" if twin else "host")
    print("host cone_eval%s: worst error / bound %.3f; finite Hessians in the recorded apex window: %s" % (" (twin)" if twin else "", worst, fin))
    assert not bad, "\n".join(bad[:20])


def test_cone_twin_against_plain(cases):
    g = cases.cone
    a, b = K.host_cone(g, False), K.host_cone(g, True)
    lim = 2 * K.cone_bounds(g)[g.fam]
    worst = 0.0
    for pi, (part, sl) in enumerate(K.CONE_PARTS):
        for i in range(g.n):
            if pi == 2 and not g.hess[i]:
                continue
            sc = max(np.abs(g.ref[i, sl]).max(), np.abs(g.alt[i]).max() if pi == 2 else 0.0)
            d = np.abs(a[i, sl] - b[i, sl]).max()
            assert d <= lim[i, pi] * sc, (g.fam_of(i), part, d, lim[i, pi] * sc)
            if sc > 0:
                worst = max(worst, d / (lim[i, pi] * sc))
    print("host cone twin vs plain: worst |difference| / (sum of bounds) %.3f" % worst)


@pytest.mark.parametrize("order,twin", ((5, False), (5, True), (6, False), (6, True)))
def test_ldl(cases, order, twin):
    g = cases.ldl(order)
    ok, L, d, x = K.host_ldl(g, order, twin)
    bad, worst = K.check_ldl(g, order, ok, L, d, x, "host/gt" if twin else "host")
    print("host ldl<%d>%s: worst error / bound %.3f" % (order, " (twin)" if twin else "", worst))
    assert not bad, "\n".join(bad[:20])


def test_cube_integrate(cases):
    final, dev = K.host_cube(cases.cube)
    bad, worst = K.check_cube(cases.cube, final, dev, "host")
    print("host cube_integrate: worst error / bound %.3f" % worst)
    assert not bad, "\n".join(bad[:20])


def test_tan_yaw_and_quat2mat(cases):
    tan, R = K.host_yaw(cases.yaw)
    bad, worst = K.check_yaw(cases.yaw, tan, R, "host")
    print("host tan_yaw / quat2mat: worst error / bound %.3f" % worst)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("family", K.YAW_FAMILIES)
def test_tan_yaw_f32_observation(cases, family):
    """(float) tan(yaw), what the observation holds, is the reference's f32 value or a neighbour; one case per family.
    The transcription of geometric_transformation.py in f64 missed this on two families - yaw within 1e-9 of +-pi/2 (m00 = 1 - (yY + zZ) cancels: 3 of 16 poses
    up to 3 f32 ulps off) and yaw = +-pi exactly (tan of the f64 pi is -+1.22e-16, the exact value 0) - which is why push_tan_yaw forms -n / d from factored
    n and d (rigid_common.h)."""
    tan, _ = K.host_yaw(cases.yaw)
    bad = K.check_yaw_f32(cases.yaw, tan, "host", family)
    assert not bad, "\n".join(bad[:20])


def test_references_regenerate(cases):
    """A sample of the stored references, evaluated again (guards the fixture against a loader or generator that drifted)."""
    c, y, l = cases.cone, cases.yaw, cases.ldl5
    for i in range(0, c.n, 37):
        assert np.array_equal(K.cone_reference(c.jar[i], *c.par[i])[0], c.ref[i])
    for i in range(0, y.n, 23):
        assert K.yaw_reference(y.q[i])[0] == y.tan[i]
    for i in range(0, l.n, 19):
        assert np.array_equal(K.ldl_reference(l.A[i], l.b[i], 5)[1], l.x[i])
    g = cases.cyl
    for i in range(0, g.n, 41):
        r = K.cyl_reference(g.pc[i], g.axis[i], g.par[i, 0], g.par[i, 1], g.pb[i], g.Rb[i], g.sb[i], g.par[i, 2])
        assert r["dist"] == g.ref_dist[i] and np.array_equal(r["out"], g.ref_out[i])
