"""k_bet_head (csrc/policy_bet.h) through d3il_bet_head_f32 on the GPU against an f64 NumPy restatement of its seven steps (LayerNorm, 64 logits, softmax numerators
and prefix sums, the uniform, the inverse-CDF bin, the offsets of the drawn bin, centre + offset -> clamp -> inverse scaling).

Shapes (a launch gets one workgroup of four waves per 32 rows, every wave walks its rows in a block-stride loop): rows 1 (a lone row, three idle waves), 63 / 64 (two
workgroups, eight passes, the last one ragged / full), 65 (a third workgroup: six passes, the last with one live wave of twelve) and 257 (nine workgroups = 36 waves, eight
passes, five live waves in the last); C in {72, 120} (both register-row instantiations, with and without a second
element per lane), A in {2, 3, 8} (partly and fully used offset groups).  Before a launch the host draws again any u within 1e-4 (of the normalised CDF) of an f64 CDF edge, so
bins are compared on every row."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V = 64
EDGE = 1e-4
SOLVER_FAIL = 1 << 16
U_MAX = np.float32(1.0 - 2.0 ** -24)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_case(rows, Cw, A, seed, logit_std=2.0):
    """Host arrays (f32) of one head problem: hidden rows, ln_f, head weights, centres, bounds, scaling, uniforms."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(h=f(rng.normal(size=(rows, Cw)) * 1.7 + 0.3), ln_w=f(1.0 + 0.3 * rng.normal(size=Cw)), ln_b=f(0.2 * rng.normal(size=Cw)), eps=1e-5,
                w=f(np.concatenate((rng.normal(size=(V, Cw)) * (logit_std / np.sqrt(Cw)), rng.normal(size=(V * A, Cw)) * (0.4 / np.sqrt(Cw))))),
                centers=f(rng.normal(size=(V, A)) * 0.9), lo=f(-1.2 - 0.3 * rng.random(A)), hi=f(1.2 + 0.3 * rng.random(A)), scale=f(0.004 * (1 + rng.random(A))),
                shift=f(0.001 * rng.normal(size=A)), u=f(rng.integers(0, 1 << 24, size=rows) / float(1 << 24)))


def head64(c, u=None, h=None):
    """The seven steps in f64 on the f32 inputs: dict(logits, probs, cdf (normalised), bins, actions)."""
    h = np.asarray(c["h"] if h is None else h, dtype=np.float64)
    u = np.asarray(c["u"] if u is None else u, dtype=np.float64)
    w, A = c["w"].astype(np.float64), c["centers"].shape[1]
    mu = h.mean(1, keepdims=True)
    x = (h - mu) / np.sqrt(((h - mu) ** 2).mean(1, keepdims=True) + c["eps"]) * c["ln_w"].astype(np.float64) + c["ln_b"].astype(np.float64)
    logits = x @ w[:V].T
    p = np.exp(logits - logits.max(1, keepdims=True))
    cs = np.cumsum(p, axis=1)
    S = cs[:, -1:]
    bins = np.minimum((cs <= u[:, None] * S).sum(1), V - 1)
    off = np.einsum("nac,nc->na", w[V + bins[:, None] * A + np.arange(A)], x)
    y = np.clip(c["centers"].astype(np.float64)[bins] + off, c["lo"], c["hi"]) * c["scale"].astype(np.float64) + c["shift"].astype(np.float64)
    return dict(x=x, logits=logits, probs=p / S, cdf=cs / S, bins=bins, actions=y)


def redraw_edges(c, seed=0):
    """Any u within EDGE of an f64 CDF edge of its row is drawn again (24-bit uniforms, as the kernel's own): returns the number of redraws."""
    rng = np.random.default_rng(1000 + seed)
    cdf = head64(c)["cdf"]
    n = 0
    for r in range(len(c["u"])):
        while np.abs(float(c["u"][r]) - cdf[r]).min() < EDGE:
            c["u"][r] = np.float32(int(rng.integers(0, 1 << 24)) / float(1 << 24)); n += 1
    return n


class Launch:
    """One call of d3il_bet_head_f32 on device copies of a case; results as host arrays.  Every pointer handed over is kept alive until the results are read."""

    def __init__(self, dev, c, u="case", seed=0, env_offset=0, t=0, probs=True, rows=None, h=None, V_=V, C_=None, t_dev=None):
        from d3il_amd import capi
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
        hh = d(c["h"] if h is None else h)
        n = hh.shape[0] if rows is None else rows
        A = c["centers"].shape[1]
        keep = [hh] + [d(c[k]) for k in ("ln_w", "ln_b", "w", "centers", "lo", "hi", "scale", "shift")]
        self.t_dev = torch.tensor([t], dtype=torch.int32, device=dev) if t_dev is None else t_dev
        u_in = d(c["u"] if isinstance(u, str) else u) if u is not None else None
        self.y = torch.full((n, A), 777.0, device=dev)
        self.b = torch.full((n,), 99, dtype=torch.int32, device=dev)
        self.uo = torch.full((n,), -5.0, device=dev)
        self.p = torch.full((n, V), -5.0, device=dev) if probs else None
        ptr = lambda x: None if x is None else x.data_ptr()
        self.rc = capi.load().d3il_bet_head_f32(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), float(c["eps"]), *(ptr(k) for k in keep[3:]), int(seed), int(env_offset), ptr(self.t_dev), ptr(u_in),
                                                ptr(self.y), ptr(self.b), ptr(self.uo), ptr(self.p), n, hh.shape[1] if C_ is None else C_, V_, A,
                                                torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        self.keep = keep + [u_in]
        self.actions, self.bins, self.u_out = self.y.cpu().numpy(), self.b.cpu().numpy(), self.uo.cpu().numpy()
        self.probs = None if self.p is None else self.p.cpu().numpy()


def torch_f32(dev, c, bins):
    """torch's own f32 layer_norm + F.linear on the same device for the same bins: (log-probabilities, actions) as f64 host arrays."""
    F = torch.nn.functional
    d = lambda a: torch.as_tensor(a).to(dev)
    A = c["centers"].shape[1]
    x = F.layer_norm(d(c["h"]), (c["h"].shape[1],), d(c["ln_w"]), d(c["ln_b"]), c["eps"])
    w = d(c["w"])
    logp = torch.log_softmax(F.linear(x, w[:V]), dim=1)
    b = torch.as_tensor(bins).to(dev)
    rows = V + b.unsqueeze(1) * A + torch.arange(A, device=dev)
    off = torch.bmm(w[rows], x.unsqueeze(2)).squeeze(2)
    y = torch.clamp(d(c["centers"])[b] + off, d(c["lo"]), d(c["hi"])) * d(c["scale"]) + d(c["shift"])
    return logp.double().cpu().numpy(), y.double().cpu().numpy()


_YARD = {}


def yardstick(dev, Cw, A):
    """Deviation of torch's f32 arithmetic from the f64 result for this (C, A), measured ONCE on the 257-row case and used for every row count: it is a property of the
    arithmetic (C-term f32 dot products behind an f32 LayerNorm), not of the number of rows, and the maximum over 257 rows is a steadier figure than that over one row."""
    if (Cw, A) not in _YARD:
        c = make_case(257, Cw, A, seed=Cw * 10 + A)
        ref = head64(c)
        logp, y = torch_f32(dev, c, ref["bins"])
        _YARD[Cw, A] = (float(np.abs(logp - np.log(ref["probs"])).max()), float(np.abs(y - ref["actions"]).max()))
    return _YARD[Cw, A]


@pytest.mark.parametrize("Cw", [72, 120])
@pytest.mark.parametrize("A", [2, 3, 8])
def test_head_equals_the_f64_restatement(dev, Cw, A):
    """Bins equal on every row; log-probabilities (= logits up to the row's log-sum) and actions within 4 x the deviation torch's own f32 layer_norm + F.linear shows
    against f64 on the same device (another summation order: lane-local chains and wave reductions instead of rocBLAS's)."""
    e_logp, e_act = yardstick(dev, Cw, A)
    for rows in (1, 63, 64, 65, 257):
        c = make_case(rows, Cw, A, seed=Cw * 10 + A)      # (the same distributions as the yardstick's case; rows = 257 IS that case)
        n_redrawn = redraw_edges(c, rows)
        ref = head64(c)
        out = Launch(dev, c)
        assert out.rc == 0
        assert np.array_equal(out.bins, ref["bins"]), (rows, np.nonzero(out.bins != ref["bins"])[0])
        assert np.array_equal(out.u_out, c["u"])
        k_logp = float(np.abs(np.log(out.probs.astype(np.float64)) - np.log(ref["probs"])).max())
        k_act = float(np.abs(out.actions.astype(np.float64) - ref["actions"]).max())
        print("C %d A %d rows %d: |log p - f64| kernel %.3e torch f32 %.3e; |action - f64| kernel %.3e torch f32 %.3e; u redrawn %d" % (Cw, A, rows, k_logp, e_logp, k_act, e_act, n_redrawn))
        assert k_logp <= 4 * e_logp and k_act <= 4 * e_act
        assert abs(float(out.probs.sum(1).max()) - 1.0) < 1e-5 and len(np.unique(ref["bins"])) > min(rows, 8) // 2
        pre = (ref["actions"] - c["shift"]) / c["scale"]
        assert rows == 1 or 0.5 < float(np.mean((pre > c["lo"] + 1e-6) & (pre < c["hi"] - 1e-6))) < 1.0      # the clamp is exercised, and is not all there is


def _extreme_case():
    """Rows: 0 = all mass in bin 0 (its logit 200 above the others': the other numerators underflow to exactly 0), 1 = all mass in bin 63, 2 = logits of magnitude
    ~80 (standard deviation 30), 3 = a row of zeros (LayerNorm of a constant row: x = ln_f's bias)."""
    c = make_case(4, 120, 3, seed=5, logit_std=0.5)
    ref = head64(c)
    x = ref["x"]
    c["w"][0] = (200.0 * x[0] / (x[0] @ x[0])).astype(np.float32)
    c["w"][63] = (200.0 * x[1] / (x[1] @ x[1])).astype(np.float32)
    x2 = x[2] / np.linalg.norm(x[2])
    c["w"][1:63] += (np.random.default_rng(6).normal(size=(62, 1)) * 30.0 * x2 / np.linalg.norm(x[2])).astype(np.float32)      # spreads row 2's logits, orthogonal-ish to rows 0 / 1
    c["h"][3] = 0.0
    return c


def test_extremes_do_not_overflow_and_the_bin_stays_inside(dev):
    c = _extreme_case()
    c["u"][:] = [0.37, 0.61, 0.5, 0.5]
    redraw_edges(c, 77)
    ref = head64(c)
    assert float(np.abs(ref["logits"][2]).max()) > 60.0 and float(ref["logits"][0].max() - np.sort(ref["logits"][0])[-2]) > 150.0
    out = Launch(dev, c)
    assert out.rc == 0 and np.isfinite(out.probs).all() and np.isfinite(out.actions).all()
    assert np.allclose(out.probs.sum(1), 1.0, atol=1e-5)
    assert out.bins.tolist() == [0, 63, int(ref["bins"][2]), int(ref["bins"][3])]
    assert float(np.abs(out.actions[2:] - ref["actions"][2:]).max()) < 1e-6 and float(np.abs(out.probs[3] - ref["probs"][3]).max()) < 1e-6
    assert out.probs[0, 0] == 1.0 and out.probs[1, 63] == 1.0 and float(out.probs[0, 1:].max()) == 0.0 and float(out.probs[1, :63].max()) == 0.0
    for u in (np.float32(0.0), U_MAX):
        o = Launch(dev, c, u=np.full(4, u, dtype=np.float32))
        assert o.bins[0] == 0 and o.bins[1] == 63, (u, o.bins)                 # never 64, never an empty leading bin
        assert (o.bins >= 0).all() and (o.bins <= 63).all() and np.isfinite(o.actions).all()
        if u == 0.0:                                                           # the first bin that holds any mass
            for r in range(4):
                assert o.probs[r, o.bins[r]] > 0.0 and float(o.probs[r, :o.bins[r]].sum()) == 0.0
        else:
            assert all(o.probs[r, o.bins[r]] > 0.0 for r in (0, 1))


def test_nonfinite_rows_are_marked_and_leave_their_neighbours_alone(dev):
    c = make_case(65, 120, 8, seed=9)
    clean = Launch(dev, c)
    h = c["h"].copy()
    h[3, 17], h[40, 100] = np.nan, np.inf
    h[64, 0] = -np.inf
    bad = Launch(dev, c, h=h)
    good = [r for r in range(65) if r not in (3, 40, 64)]
    assert bad.bins[[3, 40, 64]].tolist() == [-1, -1, -1] and np.isnan(bad.actions[[3, 40, 64]]).all()
    assert np.array_equal(bad.bins[good], clean.bins[good]) and np.array_equal(bad.actions[good], clean.actions[good]) and np.array_equal(bad.probs[good], clean.probs[good])
    assert (clean.bins >= 0).all() and np.isfinite(clean.actions).all()


def test_a_nan_row_raises_solver_fail_in_its_stacking_lane_only(dev):
    """The head's NaN action, used as the Sim uses a policy output (simulation/_rollout.py joint_rollout), for one env step of Stacking."""
    from d3il_amd.envs.stacking import CubeStackingVecEnv, load_test_contexts
    n = 6
    c = make_case(n, 120, 8, seed=10)
    c["scale"][:], c["shift"][:] = 0.003, 0.0
    h = c["h"].copy()
    h[2, 5] = np.nan
    out = Launch(dev, c, h=h)
    assert out.bins[2] == -1 and (np.delete(out.bins, 2) >= 0).all()
    env = CubeStackingVecEnv(n, device=dev, render=False, max_steps_per_episode=12)
    try:
        env.start()
        env.reset(random=False, context=load_test_contexts()[:n])
        rs = env.robot_state()
        a = out.y.to(torch.float64)
        env.step(torch.cat((a[:, :7] + rs[:, :7], a[:, 7:8]), dim=1).contiguous())
        torch.cuda.synchronize()
        fail = (env.flags[:n] & SOLVER_FAIL) != 0
        assert fail.tolist() == [r == 2 for r in range(n)]
    finally:
        env.close()


def test_philox_stream(dev):
    from d3il_amd import policies as P
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    seed, t = 0x1234567890ABCDEF, 7
    c = make_case(257, 72, 2, seed=11)
    whole = Launch(dev, c, u=None, seed=seed, env_offset=0, t=t)
    # u_out = 24 bits of Philox4x32-10(key = seed, counter = (env_offset + row, t, BET_TAG)) - the host generator is pinned by the known-answer test of tests/test_policies_bet.py
    r0 = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, np.arange(257), 0, t, P.BET_TAG)[0]
    want = (r0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(whole.u_out, want) and np.array_equal(want, P.bet_uniforms(seed, 0, 257, t))
    assert float(whole.u_out.min()) >= 0.0 and float(whole.u_out.max()) <= float(U_MAX) and len(np.unique(whole.u_out)) > 250
    # a launch on rows 100 .. 163 with env_offset 100 = the slice of the 257-row launch (row arithmetic does not depend on which wave or pass serves the row)
    part = Launch(dev, c, u=None, seed=seed, env_offset=100, t=t, h=c["h"][100:164])
    assert np.array_equal(part.u_out, whole.u_out[100:164]) and np.array_equal(part.bins, whole.bins[100:164])
    assert np.array_equal(part.actions, whole.actions[100:164]) and np.array_equal(part.probs, whole.probs[100:164])
    # the random-policy harness draws from counter word 0 for the same (seed, env, t): another stream
    env = ObstacleAvoidanceVecEnv(64, device=0)
    try:
        env.start(); env.reset(); env.policy_begin()
        tcp = env.robot_state().clone()
        act = torch.zeros(64, 7, dtype=torch.float64, device=env.device)
        env.policy_action(seed, 0, t, act)
        torch.cuda.synchronize()
        u_harness = ((act[:, 0] - tcp[:, 0] + 0.01) / 0.02).cpu().numpy()
    finally:
        env.close()
    r_h = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, np.arange(64), 0, t, 0)[0]
    assert float(np.abs(u_harness - r_h.astype(np.float64) / 2.0 ** 32).max()) < 1e-9          # that IS d3il_policy_action's first word
    assert float(np.abs(u_harness - whole.u_out[:64]).min()) > 2.0 ** -20                       # and no row of the head's stream repeats it
    # the device step word: advanced between two launches -> other numbers; the same word -> the same bits
    word = torch.tensor([t], dtype=torch.int32, device=dev)
    a = Launch(dev, c, u=None, seed=seed, t_dev=word)
    b = Launch(dev, c, u=None, seed=seed, t_dev=word)
    word.add_(1)
    d = Launch(dev, c, u=None, seed=seed, t_dev=word)
    assert np.array_equal(a.u_out, whole.u_out) and np.array_equal(a.u_out, b.u_out) and np.array_equal(a.actions, b.actions) and np.array_equal(a.bins, b.bins)
    assert not np.array_equal(d.u_out, a.u_out) and not np.array_equal(d.bins, a.bins)
    assert np.array_equal(d.u_out, P.bet_uniforms(seed, 0, 257, t + 1))


def test_unsupported_shapes_are_refused_before_any_launch(dev):
    c = make_case(4, 120, 3, seed=12)
    assert Launch(dev, c, V_=32).rc == -5 and Launch(dev, c, C_=130).rc == -5
    ok = Launch(dev, c)
    assert ok.rc == 0 and (ok.bins <= 63).all()
    untouched = Launch(dev, c, V_=32)
    assert (untouched.bins == 99).all() and (untouched.actions == 777.0).all()
