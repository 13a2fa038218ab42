"""ik_solve6 and the device-only leaf math by themselves on the GPU, through the test-only device check library (tests/devcheck): the problems, references and
bounds of tests/ik_solve6_cases.py, one problem per lane in 64-lane workgroups, compiled with the product's flags.

Shapes.  The smallest that cover what a launch can get wrong: n = 1 (one live lane), 63, 64 (one full wave), 65 (a wave and a tail of one) and 257 (four full
waves and a tail of one); a family of 64 problems (the chain: 200) fills the 257 lanes cyclically, so lanes 64 .. 256 repeat lanes 0 .. 63 in other waves and must
give the same bits.  The divergence test is one wave, the warm chain 65 lanes x 200 solves, rcpd / rsqrtd 4096 + 407 arguments in one launch, trig_advance 257 lanes x 105
increments, the controller 4 goldens x 16 lanes (+ 1) x up to 300 calls.  Nothing launches more than 257 lanes except the scalar test."""
import numpy as np
import pytest
import torch

from tests import ik_solve6_cases as K
from tests.devcheck import devcheck as D
from tests.hostcheck import hostcheck as H

pytestmark = pytest.mark.gpu
LO, HI = K.LO, K.HI
SIZES = (1, 63, 64, 65, 257)
MODES = ("jacobi", "warm", "cold")


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


def launch_solve6(A, b, vw, fast, n):
    """One launch over the first n rows; returns x, vwarm after (numpy).  vw None = the kernel without a vector."""
    dA, db, dx = dev(A[:n]), dev(b[:n]), torch.full((n, 6), float("nan"), dtype=torch.float64, device="cuda")
    dv = None if vw is None else dev(vw[:n])
    assert D.solve6(dA, db, LO, HI, dx, dv, fast, n) == 0
    torch.cuda.synchronize()
    return dx.cpu().numpy(), (None if dv is None else dv.cpu().numpy())


@pytest.fixture(scope="module")
def cases():
    return K.Cases()


@pytest.fixture(scope="module")
def dev_runs(cases):
    """Every family, every mode, every launch size; asserts the launch-size and lane-position invariance on the way.  -> {mode: (x, path)} per problem."""
    vw0 = K.warm_vectors(cases)
    out = {}
    for mode in MODES:
        x, path = np.zeros((cases.n, 6)), np.zeros(cases.n, dtype=int)
        for name in cases.names:
            s = cases.rows(name)
            m = s.stop - s.start
            idx = s.start + np.arange(257) % m
            A, b, vw = cases.A[idx], cases.b[idx], vw0[idx].copy()
            if mode == "cold":
                vw[:, 6] = 0.0
            big_x, big_v = launch_solve6(A, b, vw, mode != "jacobi", 257)
            assert np.isfinite(big_x).all(), (mode, name)
            rep = np.arange(257) % m
            assert np.array_equal(big_x, big_x[rep]) and np.array_equal(big_v, big_v[rep]), "%s/%s: a problem's result depends on its lane" % (mode, name)
            for n in SIZES[:-1]:
                sx, sv = launch_solve6(A, b, vw, mode != "jacobi", n)
                assert np.array_equal(sx, big_x[:n]) and np.array_equal(sv, big_v[:n]), "%s/%s: n = %d differs from the first rows of n = 257" % (mode, name, n)
            x[s] = big_x[:m]
            sent = big_v[:m, 6]
            if mode == "cold":
                assert np.isin(sent, (0.0, 1.0)).all()
                path[s] = np.where(sent == 1.0, 2, 0)
            else:
                path[s] = [K.path_of(v) for v in sent]
        out[mode] = (x, path)
    return out


@pytest.fixture(scope="module")
def host_runs(cases):
    vw0 = K.warm_vectors(cases)
    out = {}
    for mode in MODES:
        x, path = np.zeros((cases.n, 6)), np.zeros(cases.n, dtype=int)
        for i in range(cases.n):
            v = vw0[i].copy()
            if mode == "cold":
                v[6] = 0.0
            x[i] = H.solve6_warm(cases.A[i], cases.b[i], LO, HI, mode != "jacobi", v)
            path[i] = (2 if v[6] == 1.0 else 0) if mode == "cold" else K.path_of(v[6])
        out[mode] = (x, path)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_paths_and_accuracy(cases, dev_runs, mode):
    x, path = dev_runs[mode]
    bad = K.check(cases, x, path, "dev/" + mode, assert_path=mode != "jacobi")
    if mode == "jacobi":
        assert (path == 3).all()
    else:
        for name in ("one_0.003", "one_1e-9"):
            assert (path[cases.rows(name)] == 2).all(), name
        for name in ("b_orthogonal", "0.003_and_1.01lo"):
            s = cases.rows(name)
            print("dev/%s %s: %d deflated, %d not" % (mode, name, (path[s] == 2).sum(), (path[s] != 2).sum()))
    assert not bad, "\n".join(bad[:20])


def test_no_vector_against_cold_vector(cases, dev_runs):
    """The kernel compiled without a vector (vwarm = nullptr, the form of the older host tests) against the one with a cold vector: two instantiations, the
    compiler contracts their expressions differently, so not the same bits - within the sum of the two bounds, like device against host."""
    for fast, mode in ((True, "cold"), (False, "jacobi")):
        worst = 0.0
        for name in cases.names:
            s = cases.rows(name)
            x, _ = launch_solve6(cases.A[s], cases.b[s], None, fast, s.stop - s.start)
            d, lim = np.abs(x - dev_runs[mode][0][s]).max(axis=1), 2 * cases.bound(dev_runs[mode][1])[s]
            worst = max(worst, (d / lim).max())
            assert (d <= lim).all(), (mode, name)
        print("dev no vector vs %s vector: worst |dx| / (sum of bounds) %.3f" % (mode, worst))


def test_device_against_host(cases, dev_runs, host_runs):
    for mode in MODES:
        (xd, pd), (xh, ph) = dev_runs[mode], host_runs[mode]
        d = np.abs(xd - xh).max(axis=1)
        lim = cases.bound(pd) + cases.bound(ph)
        for name in cases.names:
            s = cases.rows(name)
            print("dev-host/%-6s %-17s largest |x_dev - x_host| / |x|_max %.2e  (/ sum of bounds %.3f)  paths differ on %d" % (
                mode, name, (d[s] / cases.xmax[s]).max(), (d[s] / lim[s]).max(), (pd[s] != ph[s]).sum()))
        assert (d <= lim).all(), np.nonzero(d > lim)


def test_fast_and_jacobi_agree(cases, dev_runs):
    xj, pj = dev_runs["jacobi"]
    for mode in ("warm", "cold"):
        xf, pf = dev_runs[mode]
        d, lim = np.abs(xf - xj).max(axis=1), cases.bound(pf) + cases.bound(pj)
        print("dev fast(%s) vs jacobi: worst |dx| / (sum of bounds) %.3f" % (mode, (d / lim).max()))
        assert (d <= lim).all()


def test_lane_independence_under_divergence(cases):
    """One wave whose lanes alternate between path-1, path-2, fall-through, guard and path-3 problems: every lane gives the bits of the same problem in a wave
    where all 64 lanes run it (what the out-of-line Jacobi and the deflation loop see in the controller wave)."""
    picks = [cases.rows(n).start for n in ("in_range", "one_0.003", "two_below", "b_orthogonal", "diagonal_lo", "ik_goldens", "one_1e-9", "trace_over_hi")]
    picks.append(cases.rows("ik_goldens").stop - 1)
    vw0 = K.warm_vectors(cases)
    for mode in ("warm", "cold"):
        idx = np.array([picks[l % len(picks)] for l in range(64)])
        vw = vw0[idx].copy()
        if mode == "cold":
            vw[:, 6] = 0.0
        mx, mv = launch_solve6(cases.A[idx], cases.b[idx], vw, True, 64)
        paths = set()
        for j, p in enumerate(picks):
            one = np.full(64, p)
            v1 = vw0[one].copy()
            if mode == "cold":
                v1[:, 6] = 0.0
            ux, uv = launch_solve6(cases.A[one], cases.b[one], v1, True, 64)
            assert np.array_equal(ux, np.tile(ux[0], (64, 1))) and np.array_equal(uv, np.tile(uv[0], (64, 1)))
            lanes = np.arange(64) % len(picks) == j
            assert np.array_equal(mx[lanes], ux[lanes]) and np.array_equal(mv[lanes], uv[lanes]), "%s: problem %d differs in the mixed wave" % (mode, p)
            paths.add(float(uv[0, 6]))
        if mode == "warm":
            assert paths == {2.0, 1.0, 0.0}      # the mixed wave really holds all three paths


def test_warm_chain(cases):
    """The 200-step chain, 65 lanes, lane e starting 7 e steps into it (lanes of a wave are at different phases: while one deflates another runs Jacobi),
    vector carried in registers; against the reference, against the same chains solved cold, and lane 0's paths against the spectrum."""
    s = cases.rows("chain")
    T, n = s.stop - s.start, 65
    t_of = (np.arange(T)[:, None] + 7 * np.arange(n)[None, :]) % T
    A, b = cases.A[s][t_of], cases.b[s][t_of]
    xref, spec = cases.x[s][t_of], cases.spec[s][t_of]
    bound = (cases.base_bound()[s] + cases.deflate_term()[s])[t_of]
    dA, db = dev(A), dev(b)
    res = {}
    for mark in (1, 0):
        dx, ds = torch.zeros((T, n, 6), dtype=torch.float64, device="cuda"), torch.full((T, n), -1.0, dtype=torch.float64, device="cuda")
        assert D.solve6_chain(dA, db, LO, HI, dx, ds, True, mark, T, n) == 0
        torch.cuda.synchronize()
        res[mark] = (dx.cpu().numpy(), ds.cpu().numpy())
    x, sent = res[1]
    assert np.array_equal(x, res[0][0])      # the marker 2.0 is as valid as 1.0: same bits
    assert np.isin(res[0][1], (0.0, 1.0)).all() and np.isin(sent, (0.0, 1.0, 2.0)).all()
    exp = np.array([[K.expected_path(sp) for sp in row] for row in spec])
    assert (sent[exp == 3] == 0.0).all()      # vwarm[6] is 0.0 after every Jacobi call
    err = np.abs(x - xref).max(axis=2)
    cold_x, _ = launch_solve6(cases.A[s], cases.b[s], np.zeros((T, 7)), True, T)
    dcold = np.abs(x - cold_x[t_of]).max(axis=2)
    # lane 0 (the chain from its start): entered warm -> exactly the spectrum's path; entered cold -> 2 may fall through to 3
    p0 = np.where(sent[:, 0] == 2.0, 1, np.where(sent[:, 0] == 1.0, 2, 0))      # 0: Jacobi, or path 1 without a vector
    entered_warm = np.r_[False, sent[:-1, 0] != 0.0]
    e0 = exp[:, 0]
    ok = (e0 == 0) | (p0 == e0) | ((p0 == 0) & ((e0 == 3) | ((e0 == 1) & ~entered_warm) | ((e0 == 2) & ~entered_warm)))
    print("dev chain: lane 0 paths 1:%d 2:%d 3|cold-1:%d, worst err/bound %.2e, worst |warm - cold| / bound %.2e" % (
        (p0 == 1).sum(), (p0 == 2).sum(), (p0 == 0).sum(), (err / bound).max(), (dcold / bound).max()))
    assert ok.all(), np.nonzero(~ok)
    assert (p0 == 2).sum() >= 50
    assert (err <= bound).all() and (dcold <= bound).all()


def _exact():
    try:
        import mpmath
        mpmath.mp.dps = 40
        return mpmath
    except ImportError:
        return None


def scalar_errors():
    """Relative errors of rcpd and rsqrtd against the exact quotient over 4096 log-uniform magnitudes in 1e-30 .. 1e30 (both signs for rcpd), the powers of two
    2^-100 .. 2^100 and 1 +- 2^-52; one launch, shared by the two tests."""
    if not scalar_errors.cache:
        rng = np.random.default_rng(11)
        mag = 10.0 ** rng.uniform(-30, 30, 4096)
        pw = 2.0 ** np.arange(-100, 101)
        pos = np.r_[mag, pw, [1 + 2.0 ** -52, 1 - 2.0 ** -52, 1.0, 3.0, 1 - 2.0 ** -53]]
        v = np.r_[pos[:2048], -pos[2048:4096], pos[4096:], -pw]
        n = len(v)
        dv, dr, dq = dev(v), torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
        assert D.scalar(dv, dr, dq, n) == 0
        torch.cuda.synchronize()
        r, q = dr.cpu().numpy(), dq.cpu().numpy()
        assert (q[v <= 0] == 0.0).all()
        mp = _exact()
        if mp is not None:
            e_r = np.array([float(abs(mp.mpf(float(a)) * mp.mpf(float(x)) - 1)) for a, x in zip(r, v)])
            e_q = np.array([float(abs(mp.mpf(float(a)) * mp.sqrt(mp.mpf(float(x))) - 1)) for a, x in zip(q, v) if x > 0])
        else:      # x87 extended precision: 64-bit significand, error 2^-64
            L = np.longdouble
            e_r = np.abs(r.astype(L) * v.astype(L) - 1).astype(float)
            e_q = np.abs(q[v > 0].astype(L) * np.sqrt(v[v > 0].astype(L)) - 1).astype(float)
        print("rcpd of the 201 powers of two: %d inexact" % (r[4096:4096 + len(pw)] != 1.0 / pw).sum())
        scalar_errors.cache.append((e_r, e_q))
    return scalar_errors.cache[0]


scalar_errors.cache = []


def test_rcpd():
    """rcpd (v_rcp_f64 + two Newton steps) against the exact quotient: relative error <= 2^-52.  Measured on MI355X: 1.110e-16 = 2^-53, the header's claim."""
    e_r, _ = scalar_errors()
    print("rcpd: max relative error %.3e (2^-53 = %.3e, header claim 1.1e-16; bound 2^-52 = %.3e)" % (e_r.max(), 2.0 ** -53, 2.0 ** -52))
    assert e_r.max() <= 2.0 ** -52


def test_rsqrtd():
    """rsqrtd (v_rsq_f64 + two Newton steps) against the exact 1 / sqrt(x): relative error <= 2^-52.
    This test found the earlier Newton step y (1.5 - 0.5 x y y) at 2.263e-16 = 1.02 x 2^-52 on MI355X (four roundings at full size); the residual form
    (r = fma(-(x y), 0.5 y, 0.5), y = fma(y, r, y)) is bounded by 0.75 x 2^-52 at the same cost.  Measured on MI355X: 1.331e-16 = 0.60 x 2^-52 (profiles/ik_solve6/README.md)."""
    _, e_q = scalar_errors()
    print("rsqrtd: max relative error %.3e (bound 2^-52 = %.3e)" % (e_q.max(), 2.0 ** -52))
    assert e_q.max() <= 2.0 ** -52


def test_trig_chain():
    """105 increments (35 sub-steps x 3 iterations) of |dl| <= 0.01 through trig_advance from angles across the joint ranges, against sin / cos of the exactly
    summed angle: 105 x 2^-52 (one rounding per product chain and step)."""
    rng = np.random.default_rng(12)
    n, Kn = 257, 105
    a0 = rng.uniform(-3.0718, 3.7525, n)
    dl = rng.uniform(-0.01, 0.01, (Kn, n))
    dl[:, 0] = 0.01; dl[:, 1] = -0.01; dl[:, 2] = 0.0; a0[3] = 0.0
    mp = _exact()
    if mp is not None:
        tot = [mp.mpf(float(a0[e])) + sum(mp.mpf(float(d)) for d in dl[:, e]) for e in range(n)]
        s0, c0 = np.array([float(mp.sin(mp.mpf(float(a)))) for a in a0]), np.array([float(mp.cos(mp.mpf(float(a)))) for a in a0])
        sr, cr = [mp.sin(t) for t in tot], [mp.cos(t) for t in tot]
        diff = lambda got, ref: np.array([float(abs(mp.mpf(float(g)) - r)) for g, r in zip(got, ref)])      # noqa: E731
    else:
        L = np.longdouble
        tot = a0.astype(L) + dl.astype(L).sum(axis=0)
        s0, c0 = np.sin(a0.astype(L)).astype(float), np.cos(a0.astype(L)).astype(float)
        sr, cr = np.sin(tot), np.cos(tot)
        diff = lambda got, ref: np.abs(got.astype(L) - ref).astype(float)      # noqa: E731
    ds, dc = dev(s0), dev(c0)
    assert D.trig_chain(dev(dl), ds, dc, Kn, n) == 0
    torch.cuda.synchronize()
    es, ec = diff(ds.cpu().numpy(), sr), diff(dc.cpu().numpy(), cr)
    print("trig_advance x %d: max |sin| error %.3e, |cos| error %.3e, bound %.3e" % (Kn, es.max(), ec.max(), Kn * 2.0 ** -52))
    assert max(es.max(), ec.max()) <= Kn * 2.0 ** -52


@pytest.mark.parametrize("form", ["product", "plain", "plain_jacobi"])
def test_ik_update_goldens(hostcheck, form):
    """The four controller goldens through ik_update on the device, 16 lanes each in one wave (lanes of a wave run sequences of different length and take
    different paths) plus one lane in a second wave; tolerances of the host test (K.golden_bounds)."""
    g = np.load(K.GOLDEN)
    lens = [g[c + "__control"].shape[0] for c in K.GOLDEN_CASES]
    n, Kmax = 65, max(lens)
    case_of = [min(e // 16, 3) for e in range(64)] + [2]
    des, jp, jv = np.zeros((Kmax, n, 7)), np.zeros((Kmax, n, 7)), np.zeros((Kmax, n, 7))
    for e, ci in enumerate(case_of):
        c, m = K.GOLDEN_CASES[ci], lens[ci]
        sp = g[c + "__setpoint"][:m]
        nq = np.sqrt(sp[:, 3] * sp[:, 3] + sp[:, 4] * sp[:, 4] + sp[:, 5] * sp[:, 5] + sp[:, 6] * sp[:, 6])      # hc_ik_control's normalisation, same order
        des[:m, e, :3], des[:m, e, 3:] = sp[:, :3], sp[:, 3:] / nq[:, None]
        jp[:m, e], jv[:m, e] = g[c + "__jpos"][:m], g[c + "__jvel"][:m]
    length = torch.as_tensor(np.array([lens[ci] for ci in case_of], dtype=np.int32), device="cuda")
    oq, ot = torch.zeros((Kmax, n, 7), dtype=torch.float64, device="cuda"), torch.zeros((Kmax, n, 7), dtype=torch.float64, device="cuda")
    prod = form == "product"
    period = hostcheck.ik_params()["n_substeps"] if prod else 0
    assert D.ik_update(dev(des), dev(jp), dev(jv), length, oq, ot, prod, prod, period, form != "plain_jacobi", n) == 0
    torch.cuda.synchronize()
    oq, ot = oq.cpu().numpy(), ot.cpu().numpy()
    for ci, c in enumerate(K.GOLDEN_CASES):
        m, lanes = lens[ci], [e for e in range(n) if case_of[e] == ci]
        for e in lanes[1:]:
            assert np.array_equal(oq[:m, e], oq[:m, lanes[0]]) and np.array_equal(ot[:m, e], ot[:m, lanes[0]]), "%s: lane %d differs from lane %d" % (c, e, lanes[0])
        bt, bq = K.golden_bounds(hostcheck, g, c, prod)
        et, eq = np.abs(ot[:m, lanes[0]] - g[c + "__control"][:m]).max(axis=1), np.abs(oq[:m, lanes[0]] - g[c + "__old_q"][:m]).max(axis=1)
        print("dev %s %s: torque %.2e (bound at the last call %.2e)  ikq %.2e (bound %.2e)" % (c, form, et.max(), bt[-1], eq.max(), bq[-1]))
        assert (et <= bt).all() and (eq <= bq).all(), (c, int(np.argmax(et > bt)), int(np.argmax(eq > bq)))


def test_refusals(cases):
    """n = 0 and NULL pointers return an error code and launch nothing (the outputs keep their bits)."""
    A, b = dev(cases.A[:64]), dev(cases.b[:64])
    x = torch.full((64, 6), 7.0, dtype=torch.float64, device="cuda")
    one = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    li = torch.ones(64, dtype=torch.int32, device="cuda")
    big = torch.full((1, 64, 7), 7.0, dtype=torch.float64, device="cuda")
    E = D.EINVAL
    assert D.solve6(A, b, LO, HI, x, None, True, 0) == E and D.solve6(A, b, LO, HI, x, None, True, -5) == E
    assert D.solve6(None, b, LO, HI, x, None, True, 64) == E and D.solve6(A, None, LO, HI, x, None, True, 64) == E and D.solve6(A, b, LO, HI, None, None, True, 64) == E
    assert D.solve6_chain(A, b, LO, HI, x, None, True, 1, 1, 64) == E and D.solve6_chain(A, b, LO, HI, x, one, True, 1, 0, 64) == E
    assert D.solve6_chain(A, b, LO, HI, x, one, True, 1, 1, 0) == E
    assert D.scalar(one, one, None, 64) == E and D.scalar(one, one, one, 0) == E and D.scalar(None, one, one, 64) == E
    assert D.trig_chain(None, one, one, 1, 64) == E and D.trig_chain(one, one, one, 0, 64) == E and D.trig_chain(one, one, one, 1, 0) == E
    assert D.ik_update(big, big, big, li, big, None, 0, 0, 0, 1, 64) == E and D.ik_update(big, big, big, None, big, big, 0, 0, 0, 1, 64) == E
    assert D.ik_update(big, big, big, li, big, big, 0, 0, 0, 1, 0) == E and D.ik_update(big, big, big, li, big, big, 1, 1, 35, 0, 64) == E
    torch.cuda.synchronize()
    assert (x == 7.0).all() and (one == 7.0).all() and (big == 7.0).all()
