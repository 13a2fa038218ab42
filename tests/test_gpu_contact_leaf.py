"""The leaf routines of the contact engines by themselves on the GPU, through the test-only device check library (tests/devcheck): box_box_emit, cyl_box,
cone_eval / gt_cone_eval, ldl_n / gt_ldl_n with their solves, cube_integrate, push_tan_yaw and quat2mat, compiled with the product's flags, one problem per lane
in 64-lane workgroups, against the stored problems, references and bounds of tests/contact_leaf_cases.py (the same checks as tests/test_contact_leaf_host.py).

Shapes.  n = 1 (one live lane), 63, 64 (one full wave), 65 (a wave and a tail of one) and 257 (four full waves and a tail of one); a family (<= 64 problems) fills
the 257 lanes cyclically, so the later waves repeat the first and must give the same bits, and a smaller launch must equal the first rows of the 257-lane one.
The divergence tests are one wave against 64-lane launches of one problem each.  Nothing launches more than 257 lanes; no test runs an episode."""
import numpy as np
import pytest
import torch

from tests import contact_leaf_cases as K
from tests.devcheck import devcheck as D

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)
NAN = float("nan")


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


def filled(shape, value, dtype=torch.float64):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def host(*ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


# ---------------------------------------------------------------- one launch per routine over the problems idx[:n]
def launch_box(g, idx, n, swapped=False, cap=8):
    A, B = (("2", "1") if swapped else ("1", "2"))
    i = idx[:n]
    a = [dev(getattr(g, k)[i]) for k in ("p" + A, "R" + A, "s" + A, "p" + B, "R" + B, "s" + B)] + [dev(g.margin[i])]
    count, rec = filled((n,), -7, torch.int32), filled((n, 8, 7), NAN)
    assert D.box_box(*a, cap, count, rec, n) == 0
    return host(count, rec)


def launch_cyl(g, idx, n):
    i = idx[:n]
    hit, out = filled((n,), -7, torch.int32), filled((n, 7), NAN)
    assert D.cyl_box(dev(g.pc[i]), dev(g.axis[i]), dev(g.par[i]), dev(g.pb[i]), dev(g.Rb[i]), dev(g.sb[i]), hit, out, n) == 0
    return host(hit, out)


def launch_cone(g, idx, n):
    i = idx[:n]
    out = filled((n, 2, 13), NAN)
    assert D.cone_eval(dev(g.jar[i]), dev(g.par[i]), out, n) == 0
    return host(out)


def launch_ldl(g, order, twin, idx, n):
    i = idx[:n]
    P = order * (order + 1) // 2
    L, d, x, ok = filled((n, P), NAN), filled((n, order), NAN), filled((n, order), NAN), filled((n,), -7, torch.int32)
    assert D.ldl(order, twin, dev(g.A[i]), dev(g.b[i]), L, d, x, ok, n) == 0
    return host(ok, L, d, x)


def launch_cube(g, idx, n, Kc, hist=True):
    i = idx[:n]
    state, qh = dev(g.state[i]), (filled((Kc, n, 4), NAN) if hist else None)
    assert D.cube_chain(state, dev(g.acc[i]), dev(g.h[i]), Kc, qh, n) == 0
    return host(state, qh) if hist else host(state)


def launch_yaw(g, idx, n):
    i = idx[:n]
    tan, R = filled((n,), NAN), filled((n, 9), NAN)
    assert D.tan_yaw(dev(g.q[i]), tan, n) == 0 and D.quat2mat(dev(g.q[i]), R, n) == 0
    return host(tan, R)


def over_families(g, launch, what, groups=None):
    """Runs every family (or the given lists of problem indices) at every launch size, asserts lane-position and launch-size invariance, and returns the
    outputs per stored problem (tuple of arrays [g.n, ...])."""
    out = None
    for name, rows in (groups or [(nm, np.arange(g.rows(nm).start, g.rows(nm).stop)) for nm in g.names]):
        m = len(rows)
        assert 0 < m <= 64
        idx = rows[np.arange(257) % m]
        big = launch(idx, 257)
        rep = np.arange(257) % m
        for b in big:
            assert np.array_equal(b, b[rep], equal_nan=True), "%s/%s: a problem's result depends on its lane" % (what, name)
        for n in SIZES[:-1]:
            for s_, b in zip(launch(idx, n), big):
                assert np.array_equal(s_, b[:n], equal_nan=True), "%s/%s: n = %d differs from the first rows of n = 257" % (what, name, n)
        if out is None:
            out = tuple(np.zeros((g.n,) + b.shape[1:], dtype=b.dtype) for b in big)
        for o, b in zip(out, big):
            o[rows] = b[:m]
    return out


@pytest.fixture(scope="module")
def cases():
    return K.Cases()


@pytest.fixture(scope="module")
def dev_box(cases):
    return {sw: over_families(cases.box, lambda idx, n: launch_box(cases.box, idx, n, sw), "box_box") for sw in (False, True)}


@pytest.fixture(scope="module")
def dev_cyl(cases):
    return over_families(cases.cyl, lambda idx, n: launch_cyl(cases.cyl, idx, n), "cyl_box")


@pytest.fixture(scope="module")
def dev_cone(cases):
    return over_families(cases.cone, lambda idx, n: launch_cone(cases.cone, idx, n), "cone_eval")[0]


@pytest.fixture(scope="module")
def dev_ldl(cases):
    return {(o, t): over_families(cases.ldl(o), lambda idx, n: launch_ldl(cases.ldl(o), o, t, idx, n), "ldl<%d>" % o) for o in (5, 6) for t in (False, True)}


# ---------------------------------------------------------------- against the references
@pytest.mark.parametrize("swapped", (False, True))
def test_box_box(cases, dev_box, swapped):
    count, rec = dev_box[swapped]
    bad, taken = K.check_box(cases.box, count, rec, "dev", swapped=swapped)
    assert not bad, "\n".join(bad[:20])


def test_box_box_cap(cases, dev_box):
    g = cases.box
    full_n, full = dev_box[False]
    rows = np.nonzero(full_n >= 4)[0][:64]
    for cap in (0, 1, 3):
        n, rec = launch_box(g, rows, len(rows), cap=cap)
        assert np.array_equal(n, np.minimum(full_n[rows], cap))
        for k, i in enumerate(rows):
            assert np.array_equal(rec[k, :n[k]], full[i, :n[k]]) and np.isnan(rec[k, n[k]:]).all()


def test_cyl_box(cases, dev_cyl):
    bad = K.check_cyl(cases.cyl, *dev_cyl, "dev")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("twin", (False, True))
def test_cone_eval(cases, dev_cone, twin):
    bad, worst, fin = K.check_cone(cases.cone, dev_cone[:, int(twin)], "dev/gt" if twin else "dev")
    print("dev cone_eval%s: worst error / bound %.3f; finite Hessians in the recorded apex window: %s" % (" (twin)" if twin else "", worst, fin))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("order,twin", ((5, False), (5, True), (6, False), (6, True)))
def test_ldl(cases, dev_ldl, order, twin):
    bad, worst = K.check_ldl(cases.ldl(order), order, *dev_ldl[(order, twin)], "dev/gt" if twin else "dev")
    print("dev ldl<%d>%s: worst error / bound %.3f" % (order, " (twin)" if twin else "", worst))
    assert not bad, "\n".join(bad[:20])


def test_cube_integrate(cases):
    g = cases.cube
    groups = [("%s/K=%d" % (nm, Kc), np.array([i for i in range(g.rows(nm).start, g.rows(nm).stop) if g.K[i] == Kc])) for nm in g.names for Kc in sorted(set(g.K[g.rows(nm)]))]
    final, dev_n = np.zeros((g.n, 13)), np.zeros(g.n)
    for name, rows in groups:
        Kc = int(g.K[rows[0]])
        (st,) = over_families(g, lambda idx, n: launch_cube(g, idx, n, Kc, hist=False), "cube_integrate", [(name, rows)])
        final[rows] = st[rows]
        st2, qh = launch_cube(g, rows, len(rows), Kc)
        assert np.array_equal(st2, st[rows]), "the chain with and without the quaternion history differs"
        assert np.array_equal(qh[-1], st2[:, 3:7])
        for k, i in enumerate(rows):      # the routine normalises only where |w| h >= 1e-15; w after call c = w0 + (c + 1) h acc
            w = g.state[i, 10:13][None] + (np.arange(Kc)[:, None] + 1) * g.h[i] * g.acc[i, 3:6][None]
            live = np.linalg.norm(w, axis=1) * g.h[i] >= 1e-15
            if live.any():
                dev_n[i] = K.quat_norm_dev(qh[live, k]).max()
    bad, worst = K.check_cube(g, final, dev_n, "dev")
    print("dev cube_integrate: worst error / bound %.3f" % worst)
    assert not bad, "\n".join(bad[:20])


@pytest.fixture(scope="module")
def dev_yaw(cases):
    return over_families(cases.yaw, lambda idx, n: launch_yaw(cases.yaw, idx, n), "tan_yaw")


def test_tan_yaw_and_quat2mat(cases, dev_yaw):
    bad, worst = K.check_yaw(cases.yaw, *dev_yaw, "dev")
    print("dev tan_yaw / quat2mat: worst error / bound %.3f" % worst)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("family", K.YAW_FAMILIES)
def test_tan_yaw_f32_observation(cases, dev_yaw, family):
    """(float) tan(yaw) is the reference's f32 value or a neighbour; one case per family (see the host test of the same name)."""
    bad = K.check_yaw_f32(cases.yaw, dev_yaw[0], "dev", family)
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------- what only a launch can get wrong
def mixed_wave(picks):
    """64 lanes that cycle through the picked problems."""
    return np.asarray(picks)[np.arange(64) % len(picks)]


def test_box_box_lanes_independent_under_divergence(cases, dev_box):
    """One wave that mixes separated pairs, inside-face contacts (4), clipped faces (5 - 8), edge contacts (1) and tie cases: every lane gives the bits of the
    same problem in a wave where all 64 lanes run it."""
    g = cases.box
    count = dev_box[False][0]
    tie = np.array([g.fam_of(i).startswith("tie_") for i in range(g.n)])
    picks = []
    for sel in (count == 0, count == 4, count == 5, count == 6, count >= 7, count == 1, count == 2, count == 3, tie):
        picks += list(np.nonzero(sel)[0][:2])
    for f in ("tie_cubes_45", "tie_edge_fudge"):
        picks.append(g.rows(f).start + 3)
    assert len(set(count[picks])) >= 7
    for sw in (False, True):
        idx = mixed_wave(picks)
        mc, mr = launch_box(g, idx, 64, sw)
        for k, i in enumerate(picks):
            uc, ur = launch_box(g, np.full(64, i), 64, sw)
            assert (uc == uc[0]).all() and np.array_equal(ur, np.broadcast_to(ur[0], ur.shape), equal_nan=True)
            for lane in range(k, 64, len(picks)):
                assert mc[lane] == uc[0] and np.array_equal(mr[lane], ur[0], equal_nan=True), "problem %d (%s) in a mixed wave" % (i, g.fam_of(i))


def test_cyl_box_lanes_independent_under_divergence(cases, dev_cyl):
    g = cases.cyl
    hit = dev_cyl[0]
    picks = list(np.nonzero(hit == 0)[0][:4]) + list(np.nonzero((hit == 1) & (g.through == 0))[0][:6]) + list(np.nonzero((hit == 1) & (g.through == 1))[0][:6])
    idx = mixed_wave(picks)
    mh, mo = launch_cyl(g, idx, 64)
    for k, i in enumerate(picks):
        uh, uo = launch_cyl(g, np.full(64, i), 64)
        assert (uh == uh[0]).all() and np.array_equal(uo, np.broadcast_to(uo[0], uo.shape), equal_nan=True)
        for lane in range(k, 64, len(picks)):
            assert mh[lane] == uh[0] and np.array_equal(mo[lane], uo[0], equal_nan=True), "problem %d (%s) in a mixed wave" % (i, g.fam_of(i))


def test_cone_eval_lanes_independent_under_divergence(cases):
    g = cases.cone
    picks = []
    for z in (-1, 0, 1, 2):      # the inert row and the three zones
        picks += list(np.nonzero(g.zone == z)[0][:4])
    picks += [g.rows("apex_1e-100").start + 1, g.rows("mu_small").start + 7]
    idx = mixed_wave(picks)
    (mo,) = launch_cone(g, idx, 64)
    for k, i in enumerate(picks):
        (uo,) = launch_cone(g, np.full(64, i), 64)
        assert np.array_equal(uo, np.broadcast_to(uo[0], uo.shape), equal_nan=True)
        for lane in range(k, 64, len(picks)):
            assert np.array_equal(mo[lane], uo[0], equal_nan=True), "problem %d (%s) in a mixed wave" % (i, g.fam_of(i))


def test_device_against_host(cases, dev_box, dev_cyl):
    """Stable box_box cases and every cyl_box case: the same count / hit and order as the host build, contacts within the sum of the two bounds."""
    g = cases.box
    for sw in (False, True):
        hc, hr = K.host_box(g, sw)
        dc, dr = dev_box[sw]
        for name in g.names:
            s = g.rows(name)
            differ = int((hc[s] != dc[s]).sum())
            same = [i for i in range(s.start, s.stop) if hc[i] == dc[i] and hc[i] > 0]
            d = max([np.abs(hr[i, :hc[i]] - dr[i, :hc[i]]).max() for i in same] or [0.0])
            print("dev-host box_box%s %-22s counts differ on %d   largest |rec_dev - rec_host| %.2e%s" % ("/swap" if sw else "", name, differ, d,
                                                                                                         "  (same count, in order)" if name.startswith("tie_") else ""))
            if not name.startswith("tie_"):
                assert differ == 0 and d <= 2 * K.ATOL, name
    g = cases.cyl
    hh, ho = K.host_cyl(g)
    dh, do = dev_cyl
    for name in g.names:
        s = g.rows(name)
        differ = int((hh[s] != dh[s]).sum())
        both = np.nonzero((hh[s] == 1) & (dh[s] == 1))[0] + s.start
        d = np.abs(ho[both] - do[both]).max() if len(both) else 0.0
        print("dev-host cyl_box %-14s hit differs on %d   largest |out_dev - out_host| %.2e" % (name, differ, d))
        assert differ == 0 and d <= 2 * K.ATOL, name


def test_twin_against_plain(cases, dev_cone, dev_ldl):
    """cone_eval against gt_cone_eval (one launch) and ldl_n against gt_ldl_n: within the sum of the two bounds."""
    g = cases.cone
    lim = 2 * K.cone_bounds(g)[g.fam]
    worst = 0.0
    for pi, (part, sl) in enumerate(K.CONE_PARTS):
        for i in range(g.n):
            if pi == 2 and not g.hess[i]:
                continue
            sc = max(np.abs(g.ref[i, sl]).max(), np.abs(g.alt[i]).max() if pi == 2 else 0.0)
            d = np.abs(dev_cone[i, 0, sl] - dev_cone[i, 1, sl]).max()
            assert d <= lim[i, pi] * sc, (g.fam_of(i), part, d, lim[i, pi] * sc)
            if sc > 0:
                worst = max(worst, d / (lim[i, pi] * sc))
    print("dev cone twin vs plain: worst |difference| / (sum of bounds) %.3f; bit-identical on %d of %d problems" % (
        worst, sum(np.array_equal(dev_cone[i, 0], dev_cone[i, 1], equal_nan=True) for i in range(g.n)), g.n))
    for order in (5, 6):
        g = cases.ldl(order)
        (ok0, _, _, x0), (ok1, _, _, x1) = dev_ldl[(order, False)], dev_ldl[(order, True)]
        assert np.array_equal(ok0, ok1)
        lim = 2 * K.ldl_bounds(g)[g.fam]
        live = g.ok.astype(bool)
        r = np.abs(x0 - x1).max(axis=1)[live] / (lim[live] * np.abs(g.x[live]).max(axis=1))
        print("dev ldl<%d> twin vs plain: worst |dx| / (sum of bounds) %.3f" % (order, r.max()))
        assert (r <= 1).all()


def test_refusals(cases):
    """n = 0, a negative n and a NULL required pointer: DC_EINVAL, nothing launched, the outputs untouched."""
    b, c, o, l, q, y = cases.box, cases.cyl, cases.cone, cases.ldl5, cases.cube, cases.yaw
    i = np.arange(4)
    count, rec = filled((4,), -7, torch.int32), filled((4, 8, 7), 3.5)
    box_in = [dev(getattr(b, k)[i]) for k in ("p1", "R1", "s1", "p2", "R2", "s2", "margin")]
    hit, out7 = filled((4,), -7, torch.int32), filled((4, 7), 3.5)
    cyl_in = [dev(getattr(c, k)[i]) for k in ("pc", "axis", "par", "pb", "Rb", "sb")]
    cone_out = filled((4, 2, 13), 3.5)
    L, d, x, ok = filled((4, 15), 3.5), filled((4, 5), 3.5), filled((4, 5), 3.5), filled((4,), -7, torch.int32)
    state0 = dev(q.state[i])
    state, tan, R = state0.clone(), filled((4,), 3.5), filled((4, 9), 3.5)
    for n in (0, -1, -64):
        assert D.box_box(*box_in, 8, count, rec, n) == D.EINVAL
        assert D.cyl_box(*cyl_in, hit, out7, n) == D.EINVAL
        assert D.cone_eval(dev(o.jar[i]), dev(o.par[i]), cone_out, n) == D.EINVAL
        assert D.ldl(5, 0, dev(l.A[i]), dev(l.b[i]), L, d, x, ok, n) == D.EINVAL
        assert D.cube_chain(state, dev(q.acc[i]), dev(q.h[i]), 3, None, n) == D.EINVAL
        assert D.tan_yaw(dev(y.q[i]), tan, n) == D.EINVAL and D.quat2mat(dev(y.q[i]), R, n) == D.EINVAL
    for k in range(7):
        a = list(box_in)
        a[k] = None
        assert D.box_box(*a, 8, count, rec, 4) == D.EINVAL
    assert D.box_box(*box_in, 8, None, rec, 4) == D.EINVAL and D.box_box(*box_in, 8, count, None, 4) == D.EINVAL
    for k in range(6):
        a = list(cyl_in)
        a[k] = None
        assert D.cyl_box(*a, hit, out7, 4) == D.EINVAL
    assert D.cyl_box(*cyl_in, None, out7, 4) == D.EINVAL and D.cyl_box(*cyl_in, hit, None, 4) == D.EINVAL
    assert D.cone_eval(None, dev(o.par[i]), cone_out, 4) == D.EINVAL and D.cone_eval(dev(o.jar[i]), None, cone_out, 4) == D.EINVAL
    assert D.cone_eval(dev(o.jar[i]), dev(o.par[i]), None, 4) == D.EINVAL
    assert D.ldl(4, 0, dev(l.A[i]), dev(l.b[i]), L, d, x, ok, 4) == D.EINVAL and D.ldl(5, 0, None, dev(l.b[i]), L, d, x, ok, 4) == D.EINVAL
    assert D.ldl(5, 0, dev(l.A[i]), dev(l.b[i]), L, d, x, None, 4) == D.EINVAL and D.ldl(5, 1, dev(l.A[i]), dev(l.b[i]), None, d, x, ok, 4) == D.EINVAL
    assert D.cube_chain(None, dev(q.acc[i]), dev(q.h[i]), 3, None, 4) == D.EINVAL and D.cube_chain(state, dev(q.acc[i]), dev(q.h[i]), 0, None, 4) == D.EINVAL
    assert D.cube_chain(state, None, dev(q.h[i]), 3, None, 4) == D.EINVAL and D.cube_chain(state, dev(q.acc[i]), None, 3, None, 4) == D.EINVAL
    assert D.tan_yaw(None, tan, 4) == D.EINVAL and D.tan_yaw(dev(y.q[i]), None, 4) == D.EINVAL
    assert D.quat2mat(None, R, 4) == D.EINVAL and D.quat2mat(dev(y.q[i]), None, 4) == D.EINVAL
    torch.cuda.synchronize()
    assert (count == -7).all() and (hit == -7).all() and (ok == -7).all() and torch.equal(state, state0)
    for t in (rec, out7, cone_out, L, d, x, tan, R):
        assert (t == 3.5).all()
