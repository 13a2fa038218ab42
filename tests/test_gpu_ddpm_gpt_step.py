"""k_ddpm_gpt_step (csrc/policy_ddpm_gpt.h) through d3il_ddpm_gpt_step_f32 on the GPU against an f64 NumPy restatement of its eight steps (LayerNorm, the linear head,
clipped x0, posterior mean, noise, the next iterate, its action tokens + the time token, at chain index 0 the clamped and inverse-scaled action).

Geometry (a launch gets one workgroup of four waves per 8 environments, at most 1024 workgroups; one wave owns one environment at a time and walks its W positions,
every wave takes its environments in a block-stride loop): n_env 1 (a lone environment, three idle waves), 63 (8 workgroups = 32 waves, two passes, the second with 31
live waves: one short of a multiple of what a pass of 8 workgroups holds), 64 (two full passes), 65 (a ninth workgroup: 36 waves, 29 live in the second pass), 257
(33 workgroups = 132 waves, 125 live in the second pass) and 8200 (the capped grid, three passes).
C in {72, 120} are the compile-time widths, C in {32, 100, 128} run the run-time instantiation (32: no second element per lane, half the lanes idle; the golden net's
width); A in {2, 3, 8}; W in {1, 5}; chain index k in {T (init), T - 1, 1, 0}; ragged lengths 1 .. W."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = 8
SOLVER_FAIL = 1 << 16
SENT = 777.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def schedule(t):
    from d3il_amd import policies as P
    betas = P.cosine_beta_schedule(t)
    alphas = 1.0 - betas
    ac = torch.cumprod(alphas, dim=0)
    ac_prev = torch.cat([torch.ones(1), ac[:-1]])
    sig = (0.5 * torch.log(torch.clamp(betas * (1.0 - ac_prev) / (1.0 - ac), min=1e-20))).exp() * torch.cat((torch.zeros(1), torch.ones(t - 1)))
    return torch.stack((torch.sqrt(1.0 / ac), torch.sqrt(1.0 / ac - 1), betas * torch.sqrt(ac_prev) / (1.0 - ac), (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac), sig), dim=1).numpy()


def make_case(n, W, Cw, A, seed):
    """Host arrays (f32) of one problem: hidden rows, ln_f, head, action embedding, tables, bounds, scaling, ragged lengths, iterate, noise."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(hk=f(rng.normal(size=(n, W, Cw)) * 1.7 + 0.3), ln_w=f(1.0 + 0.3 * rng.normal(size=Cw)), ln_b=f(0.2 * rng.normal(size=Cw)), eps=1e-5,
                w_pred=f(rng.normal(size=(A, Cw)) / np.sqrt(Cw)), b_pred=f(0.1 * rng.normal(size=A)), w_aemb=f(rng.normal(size=(Cw, A)) * 0.3),
                bias_pos=f(rng.normal(size=(W, Cw)) * 0.2), temb=f(rng.normal(size=(T, Cw)) * 0.5), sched=f(schedule(T)), lo=f(-1.2 - 0.3 * rng.random(A)),
                hi=f(1.2 + 0.3 * rng.random(A)), scale=f(0.004 * (1 + rng.random(A))), shift=f(0.001 * rng.normal(size=A)),
                len=np.ascontiguousarray(1 + (np.arange(n) * 7 + seed) % W, dtype=np.int64), x=f(rng.normal(size=(n, W, A))), noise=f(rng.normal(size=(n, W, A))))


def first_rows(c, n):
    """The case cut down to its first n environments."""
    return dict(c, **{q: np.ascontiguousarray(c[q][:n]) for q in ("hk", "len", "x", "noise")})


def step64(c, k, noise=None, hk=None, x=None):
    """The eight steps in f64 on the f32 inputs: dict(xp [n, W, A], tok [n, W, C], actions [n, A] (k = 0), valid [n, W])."""
    d = lambda a: np.asarray(a, dtype=np.float64)
    n, W, A = c["x"].shape
    noise = d(c["noise"] if noise is None else noise)
    valid = np.arange(W)[None, :] < c["len"][:, None]
    if k == T:
        xp = noise
    else:
        h, x = d(c["hk"] if hk is None else hk), d(c["x"] if x is None else x)
        mu = h.mean(2, keepdims=True)
        z = (h - mu) / np.sqrt(((h - mu) ** 2).mean(2, keepdims=True) + c["eps"]) * d(c["ln_w"]) + d(c["ln_b"])
        eps = z @ d(c["w_pred"]).T + d(c["b_pred"])
        s = d(c["sched"][k])
        x0 = np.clip(s[0] * x - s[1] * eps, d(c["lo"]), d(c["hi"]))
        mean = s[2] * x0 + s[3] * x
        xp = mean if k == 0 else mean + s[4] * noise
    xp = np.where(valid[:, :, None], xp, 0.0)
    out = dict(xp=xp, valid=valid, tok=xp @ d(c["w_aemb"]).T + d(c["bias_pos"]))
    if k == 0:
        last = xp[np.arange(n), c["len"] - 1]
        out["actions"] = np.clip(last, d(c["lo"]), d(c["hi"])) * d(c["scale"]) + d(c["shift"])
    return out


def torch_f32(dev, c, k):
    """torch's own f32 layer_norm + F.linear chain on the same device for the same case: (xp, tok, actions or None) as f64 host arrays."""
    F = torch.nn.functional
    d = lambda a: torch.as_tensor(a).to(dev)
    n, W, A = c["x"].shape
    valid = (torch.arange(W, device=dev)[None, :] < d(c["len"])[:, None]).unsqueeze(2)
    if k == T:
        xp = d(c["noise"])
    else:
        z = F.layer_norm(d(c["hk"]), (c["hk"].shape[2],), d(c["ln_w"]), d(c["ln_b"]), c["eps"])
        eps = F.linear(z, d(c["w_pred"]), d(c["b_pred"]))
        s, x = d(c["sched"][k]), d(c["x"])
        x0 = torch.minimum(torch.maximum(s[0] * x - s[1] * eps, d(c["lo"])), d(c["hi"]))
        mean = s[2] * x0 + s[3] * x
        xp = mean if k == 0 else mean + s[4] * d(c["noise"])
    xp = torch.where(valid, xp, torch.zeros_like(xp))
    tok = F.linear(xp, d(c["w_aemb"])) + d(c["bias_pos"])
    act = None
    if k == 0:
        last = xp[torch.arange(n, device=dev), d(c["len"]) - 1]
        act = (torch.minimum(torch.maximum(last, d(c["lo"])), d(c["hi"])) * d(c["scale"]) + d(c["shift"])).double().cpu().numpy()
    return xp.double().cpu().numpy(), tok.double().cpu().numpy(), act


class Launch:
    """One call of d3il_ddpm_gpt_step_f32 on device copies of a case; results as host arrays.  Every pointer handed over is kept alive until the results are read.
    ``state``: (x, xbuf, actions, bad) device tensors of an earlier launch to go on with (a chain), otherwise fresh ones filled with sentinels."""

    def __init__(self, dev, c, k, noise="case", seed=0, env_offset=0, t=0, t_dev=None, hk=None, x=None, state=None, want_noise=True, C_=None, A_=None, W_=None, T_=T, n_=None):
        from d3il_amd import capi
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
        n, W, A = c["x"].shape
        Cw = c["hk"].shape[2]
        n = n if n_ is None else n_
        keep = [d(c["hk"] if hk is None else hk)] + [d(c[q]) for q in ("ln_w", "ln_b", "w_pred", "b_pred", "w_aemb", "bias_pos", "temb", "sched", "lo", "hi", "scale", "shift", "len")]
        self.t_dev = torch.tensor([t], dtype=torch.int32, device=dev) if t_dev is None else t_dev
        n_in = None if noise is None else d(c["noise"] if isinstance(noise, str) else noise)
        if state is None:
            self.x = d(c["x"] if x is None else x).clone()
            self.xbuf = torch.full((n, 2 * W + 1, Cw), SENT, device=dev)
            self.act = torch.full((n, A), SENT, device=dev)
            self.bad_t = torch.full((n,), 0 if k < T else 99, dtype=torch.int32, device=dev)
        else:
            self.x, self.xbuf, self.act, self.bad_t = state
        self.x_in = self.x.cpu().numpy().copy()
        self.no = torch.full((n, W, A), SENT, device=dev) if want_noise else None
        ptr = lambda v: None if v is None else v.data_ptr()
        self.rc = capi.load().d3il_ddpm_gpt_step_f32(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), float(c["eps"]), *(ptr(q) for q in keep[3:]), int(seed), int(env_offset), ptr(self.t_dev),
                                                     ptr(n_in), ptr(self.x), ptr(self.xbuf), ptr(self.act), ptr(self.bad_t), ptr(self.no), n, Cw if C_ is None else C_,
                                                     A if A_ is None else A_, W if W_ is None else W_, T_, k, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        self.keep = keep + [n_in]
        self.state = (self.x, self.xbuf, self.act, self.bad_t)
        self.x_out, self.buf, self.actions, self.bad = self.x.cpu().numpy(), self.xbuf.cpu().numpy(), self.act.cpu().numpy(), self.bad_t.cpu().numpy()
        self.noise_out = None if self.no is None else self.no.cpu().numpy()


_FULL = {}


def full_case(dev, W, Cw, A, k):
    """(case, f64 result, launch) of the 257-environment problem of this (W, C, A, k): computed once, shared, left unchanged."""
    if (W, Cw, A, k) not in _FULL:
        c = make_case(257, W, Cw, A, seed=Cw * 10 + A)
        _FULL[W, Cw, A, k] = (c, step64(c, k), Launch(dev, c, k))
    return _FULL[W, Cw, A, k]


def check_against_f64(dev, c, ref, out, k):
    """One launch against the f64 restatement of ITS case: x', the token rows and the actions within 4 x the deviation of torch's own f32 chain on the same device for
    the same case; plus what the launch must and must not write."""
    n, W, A = c["x"].shape
    Cw = c["hk"].shape[2]
    t_x, t_tok, t_act = torch_f32(dev, c, k)
    e_x, e_tok = float(np.abs(t_x - ref["xp"]).max()), float(np.abs(t_tok - ref["tok"]).max())
    assert out.rc == 0
    assert np.array_equal(out.noise_out, c["noise"]) and (out.bad == 0).all()
    tok = out.buf[:, 2::2]
    if k > 0:
        k_x, k_tok = float(np.abs(out.x_out - ref["xp"]).max()), float(np.abs(tok - ref["tok"]).max())
        print("n %d W %d C %d A %d k %d: |x' - f64| kernel %.3e torch f32 %.3e; |token - f64| kernel %.3e torch f32 %.3e" % (n, W, Cw, A, k, k_x, e_x, k_tok, e_tok))
        assert k_x <= 4 * e_x and k_tok <= 4 * e_tok
        assert np.array_equal(out.buf[:, 0], np.broadcast_to(c["temb"][k - 1], (n, Cw)))      # the time token of the NEXT chain step
        assert (out.buf[:, 1::2] == SENT).all() and (out.actions == SENT).all()                 # the state tokens and the action are not this launch's
        pad = ~ref["valid"]
        assert (out.x_out[pad] == 0.0).all() and np.array_equal(tok[pad], np.broadcast_to(c["bias_pos"][None], tok.shape)[pad])
        assert W == 1 or pad.any()
    else:
        e_act = float(np.abs(t_act - ref["actions"]).max())
        k_act = float(np.abs(out.actions - ref["actions"]).max())
        print("n %d W %d C %d A %d k 0: |action - f64| kernel %.3e torch f32 %.3e" % (n, W, Cw, A, k_act, e_act))
        assert k_act <= 4 * e_act
        assert np.array_equal(out.x_out, c["x"]) and (out.buf == SENT).all()                  # chain index 0 writes the action only
        pre = (ref["actions"] - c["shift"]) / c["scale"]
        assert 0.2 < float(np.mean((pre > c["lo"] + 1e-4) & (pre < c["hi"] - 1e-4))) < 1.0      # the clamp is exercised, and is not all there is


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("Cw", [72, 120])
@pytest.mark.parametrize("A", [2, 3, 8])
@pytest.mark.parametrize("W", [1, 5])
def test_step_equals_the_f64_restatement(dev, W, A, Cw):
    """The 257-environment launch: x', the token rows and the actions within 4 x the deviation torch's own f32 layer_norm + F.linear chain shows against f64 on the same
    device for the same 257 environments (another summation order: wave reductions and lane-local chains instead of rocBLAS's; in init mode x' IS the noise, deviation
    0: bit equality).  The launches of 1 / 63 / 64 / 65 environments run the first rows of that case and must give those rows of the 257 launch BIT FOR BIT - x',
    every token row, the action, the noise, the flag: an environment's result does not depend on which wave, workgroup or pass serves it, so the bar that holds for
    the 257 rows holds for every smaller launch row by row (a pooled bar would not: at k = T - 1 the deviation is carried by a few ill-conditioned rows)."""
    for k in (T, T - 1, 1, 0):
        c, ref, full = full_case(dev, W, Cw, A, k)
        check_against_f64(dev, c, ref, full, k)
        for n in (1, 63, 64, 65):
            out = Launch(dev, first_rows(c, n), k)
            assert out.rc == 0
            for name in ("x_out", "buf", "actions", "noise_out", "bad"):
                assert np.array_equal(bits(getattr(out, name)), bits(getattr(full, name)[:n])), (n, k, name)


@pytest.mark.parametrize("Cw", [32, 100, 128])
def test_run_time_width_instantiation(dev, Cw):
    for k in (T, 3, 0):
        c, ref, full = full_case(dev, 5, Cw, 8, k)
        check_against_f64(dev, c, ref, full, k)


def test_three_passes_behind_the_grid_cap(dev):
    """8200 environments: the grid is capped at 1024 workgroups = 4096 waves, so every wave makes three passes, the third with 8 live waves.  Same bar, on this case;
    and the first 257 environments equal a 257-environment launch bit for bit."""
    for k in (T - 1, 0):
        c = make_case(8200, 1, 72, 2, seed=31)
        out = Launch(dev, c, k)
        check_against_f64(dev, c, step64(c, k), out, k)
        small = Launch(dev, first_rows(c, 257), k)
        for name in ("x_out", "buf", "actions"):
            assert np.array_equal(bits(getattr(small, name)), bits(getattr(out, name)[:257])), (k, name)


def test_clamp_edges_are_exact(dev):
    """coef1 = 1, coef2 = 0, sig = 0: x' = x0.  The head's bias pushes x0 far below the lower bound on component 0 and far above the upper one on component 1: those
    come out as the bounds, bit for bit; the other components stay strictly inside (and within the usual bar)."""
    c = make_case(65, 5, 120, 8, seed=3)
    c["sched"][4] = [1.0, 1.0, 1.0, 0.0, 0.0]
    c["b_pred"][0], c["b_pred"][1] = 50.0, -50.0
    c["x"] *= 0.15; c["w_pred"][2:] *= 0.15; c["b_pred"][2:] = 0.0
    ref = step64(c, 4)
    out = Launch(dev, c, 4)
    v = ref["valid"]
    assert out.rc == 0 and v.sum() > 100
    assert (out.x_out[v][:, 0] == c["lo"][0]).all() and (out.x_out[v][:, 1] == c["hi"][1]).all()
    inner = out.x_out[v][:, 2:]
    assert (inner > c["lo"][2:]).all() and (inner < c["hi"][2:]).all() and float(np.abs(inner - ref["xp"][v][:, 2:]).max()) < 1e-5
    # and the final clamp of chain index 0, with a posterior mean beyond the bounds: coef1 = 2
    c["sched"][0] = [1.0, 1.0, 2.0, 0.0, 0.0]
    c["scale"][:], c["shift"][:] = 1.0, 0.0
    o0 = Launch(dev, c, 0)
    assert (o0.actions[:, 0] == c["lo"][0]).all() and (o0.actions[:, 1] == c["hi"][1]).all()


def test_chain_index_zero_ignores_its_noise(dev):
    c = make_case(65, 5, 120, 8, seed=4)
    a = Launch(dev, c, 0, noise=np.zeros_like(c["noise"]))
    b = Launch(dev, c, 0, noise=np.full_like(c["noise"], 1e30))
    d = Launch(dev, c, 0, noise=None)
    assert np.array_equal(a.actions.view(np.uint32), b.actions.view(np.uint32)) and np.array_equal(a.actions.view(np.uint32), d.actions.view(np.uint32))
    assert np.isfinite(a.actions).all() and (d.noise_out == 0.0).all()      # nothing is drawn at chain index 0


def run_chain(dev, c, hks, poison=None):
    """Init launch, then chain indices T - 1 .. 0 on one state, hidden rows hks[k]; ``poison`` = (k, env, position, element, value) is put into that launch's rows.
    Returns the launches by chain index."""
    out = {T: Launch(dev, c, T)}
    state = out[T].state
    for k in reversed(range(T)):
        hk = hks[k]
        if poison is not None and poison[0] == k:
            hk = hk.copy()
            hk[poison[1], poison[2], poison[3]] = poison[4]
        out[k] = Launch(dev, c, k, hk=hk, state=state)
    return out


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("when", [T - 1, 3])
def test_nonfinite_rows_mark_their_environment_and_leave_the_neighbours_alone(dev, when, value):
    """A NaN / an Inf in one environment's hidden rows at the first / at a middle chain step: that environment's action is NaN, ``bad`` is sticky across the launches
    that follow (their hidden rows are clean), every other environment is bit-equal to a clean chain; a NaN at a PADDED position marks nothing."""
    n, W, Cw, A = 65, 5, 120, 8
    c = make_case(n, W, Cw, A, seed=9)
    rng = np.random.default_rng(19)
    hks = {k: (rng.normal(size=(n, W, Cw)) * 1.7 + 0.3).astype(np.float32) for k in range(T)}
    e = 40
    assert c["len"][e] >= 1 and c["len"][7] < W
    clean = run_chain(dev, c, hks)
    dirty = run_chain(dev, c, hks, poison=(when, e, 0, 17, value))
    others = np.arange(n) != e
    assert clean[T].bad.tolist() == [0] * n and (clean[0].bad == 0).all() and np.isfinite(clean[0].actions).all()
    for k in range(T - 1, -1, -1):
        assert (dirty[k].bad[others] == 0).all() and int(dirty[k].bad[e]) == (1 if k <= when else 0), k
    assert np.isnan(dirty[0].actions[e]).all()
    assert np.array_equal(dirty[0].actions[others].view(np.uint32), clean[0].actions[others].view(np.uint32))
    assert np.array_equal(dirty[1].x_out[others].view(np.uint32), clean[1].x_out[others].view(np.uint32))
    assert np.array_equal(dirty[1].buf[others].view(np.uint32), clean[1].buf[others].view(np.uint32))
    padded = run_chain(dev, c, hks, poison=(when, 7, W - 1, 3, value))
    assert (padded[0].bad == 0).all() and np.array_equal(padded[0].actions.view(np.uint32), clean[0].actions.view(np.uint32))
    # the init launch clears the flag
    again = Launch(dev, c, T, state=dirty[0].state)
    assert (again.bad == 0).all()


def test_a_bad_environment_raises_solver_fail_in_its_stacking_lane_only(dev):
    """The kernel's NaN action, used as the Sim uses a policy output (simulation/_rollout.py joint_rollout), for one env step of Stacking."""
    from d3il_amd.envs.stacking import CubeStackingVecEnv, load_test_contexts
    n = 6
    c = make_case(n, 5, 120, 8, seed=10)
    c["scale"][:], c["shift"][:] = 0.003, 0.0
    hk = c["hk"].copy()
    hk[2, 0, 5] = np.nan
    out = Launch(dev, c, 0, hk=hk)
    assert out.bad.tolist() == [0, 0, 1, 0, 0, 0] and np.isnan(out.actions[2]).all() and np.isfinite(np.delete(out.actions, 2, axis=0)).all()
    env = CubeStackingVecEnv(n, device=dev, render=False, max_steps_per_episode=12)
    try:
        env.start()
        env.reset(random=False, context=load_test_contexts()[:n])
        rs = env.robot_state()
        a = out.act.to(torch.float64)
        env.step(torch.cat((a[:, :7] + rs[:, :7], a[:, 7:8]), dim=1).contiguous())
        torch.cuda.synchronize()
        fail = (env.flags[:n] & SOLVER_FAIL) != 0
        assert fail.tolist() == [r == 2 for r in range(n)]
    finally:
        env.close()


def test_philox_stream(dev):
    from d3il_amd import policies as P
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    from tests.test_gpu_bet_head import Launch as BetLaunch, make_case as bet_case
    seed, t, k, n, W, A = 0x1234567890ABCDEF, 7, 5, 257, 5, 8
    c = make_case(n, W, 72, A, seed=11)
    whole = Launch(dev, c, k, noise=None, seed=seed, t=t)
    want = P.ddpm_gpt_normals(seed, 0, n, t, k, W, A)
    # the yardstick: torch's f32 evaluation of the same Box-Muller formula on the same words, on the device
    w = torch.as_tensor(P.ddpm_gpt_words(seed, 0, n, t, k, W).astype(np.int64)).to(dev)
    u1 = ((w[..., 0::2] >> 8) + 1).float() * (2.0 ** -24)
    u2 = (w[..., 1::2] >> 8).float() * (2.0 ** -24)
    rad, ang = torch.sqrt(-2.0 * torch.log(u1)), 6.283185307179586 * u2
    z32 = torch.stack((rad * torch.cos(ang), rad * torch.sin(ang)), dim=-1).reshape(n, W, 8)[:, :, :A].double().cpu().numpy()
    e32, e_k = float(np.abs(z32 - want).max()), float(np.abs(whole.noise_out - want).max())
    print("Box-Muller against f64: kernel %.3e, torch f32 %.3e; largest |normal| %.2f" % (e_k, e32, float(np.abs(want).max())))
    assert e_k <= 4 * e32 and np.isfinite(whole.noise_out).all()
    # the launch used what it reports: x' = mean + sig * noise_out, against a launch that gets the same numbers handed in
    fed = Launch(dev, c, k, noise=whole.noise_out)
    assert np.array_equal(fed.x_out, whole.x_out) and np.array_equal(fed.buf, whole.buf)
    # a launch on environments 100 .. 163 with env_offset 100 = the slice of the 257-environment launch
    sl = slice(100, 164)
    part_case = dict(c, hk=c["hk"][sl], x=c["x"][sl], len=c["len"][sl], noise=c["noise"][sl])
    part = Launch(dev, part_case, k, noise=None, seed=seed, env_offset=100, t=t)
    assert np.array_equal(part.noise_out, whole.noise_out[sl]) and np.array_equal(part.x_out, whole.x_out[sl]) and np.array_equal(part.buf, whole.buf[sl])
    # other chain indices and the init mode draw other numbers; the A = 3 launch draws the first three components of the same words
    init = Launch(dev, c, T, noise=None, seed=seed, t=t)
    assert float(np.abs(init.noise_out - P.ddpm_gpt_normals(seed, 0, n, t, T, W, A)).max()) <= 4 * e32 and not np.array_equal(init.noise_out, whole.noise_out)
    assert np.array_equal(init.x_out[step64(c, T)["valid"]], init.noise_out[step64(c, T)["valid"]])
    # BeT's head and the random-policy harness draw from other counter words for the same (seed, environment, t): their first words never meet ours
    ours = ((P.ddpm_gpt_words(seed, 0, n, t, k, W)[..., 0] >> np.uint32(8)).astype(np.float64)) * 2.0 ** -24      # [n, W, 2]
    bc = bet_case(n, 72, 2, seed=11)
    bet = BetLaunch(dev, bc, u=None, seed=seed, env_offset=0, t=t)
    assert np.array_equal(bet.u_out, P.bet_uniforms(seed, 0, n, t))
    assert float(np.abs(ours - bet.u_out.astype(np.float64)[:, None, None]).min()) > 0.0
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
    assert float(np.abs(ours[:64] - u_harness[:, None, None]).min()) > 2.0 ** -24
    # the device step word: advanced between two launches -> other numbers; the same word -> the same bits
    word = torch.tensor([t], dtype=torch.int32, device=dev)
    a = Launch(dev, c, k, noise=None, seed=seed, t_dev=word)
    b = Launch(dev, c, k, noise=None, seed=seed, t_dev=word)
    word.add_(1)
    d = Launch(dev, c, k, noise=None, seed=seed, t_dev=word)
    assert np.array_equal(a.noise_out, whole.noise_out) and np.array_equal(a.noise_out, b.noise_out) and np.array_equal(a.x_out, b.x_out)
    assert not np.array_equal(d.noise_out, a.noise_out)
    assert float(np.abs(d.noise_out - P.ddpm_gpt_normals(seed, 0, n, t + 1, k, W, A)).max()) <= 4 * e32


def test_unsupported_shapes_are_refused_before_any_launch(dev):
    c = make_case(4, 5, 120, 3, seed=12)
    for kw in (dict(C_=130), dict(C_=122), dict(A_=9), dict(A_=0), dict(W_=17), dict(T_=256)):
        out = Launch(dev, c, 3, **kw)
        assert out.rc == -5, kw
        assert (out.buf == SENT).all() and (out.actions == SENT).all() and np.array_equal(out.x_out, c["x"]) and (out.noise_out == SENT).all(), kw
    ok = Launch(dev, c, 3)
    assert ok.rc == 0 and (ok.buf[:, 0] != SENT).all()
