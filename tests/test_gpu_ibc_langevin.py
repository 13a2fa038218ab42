"""k_ibc_langevin (csrc/policy_ibc.h) through d3il_ibc_langevin_f32 on the GPU against an f64 torch restatement of its three steps (start points, K Langevin
iterations with the gradient of the energy network, the energies of the final samples + one categorical draw); all banks given unless the test is about Philox.

Geometry: one workgroup of eight waves per environment, its four row tiles of 16 samples one after the other - so every launch with n_env >= 1 runs every path;
n_env 1, 3, 4, 16 and 17 are compared row by row.  The grid is the environment count (not capped).  Shapes: hidden 128 with 1 and 3 blocks (one output tile per
wave), hidden 256 with 4 blocks (two tiles per wave, all four derivative register sets); (obs, A) = (4, 2), (20, 3), (20, 8) (A = 8: obs + A = 28 fills the seven-step
input layer, the second Philox call).  Yardsticks are torch's own f32 autograd evaluation of the same rows (its own layers, on the same device), taken per case and never carried over."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SOLVER_FAIL = 1 << 16
N, S, K, EDGE = 17, 64, 20, 1e-4
CASES = {"h128b1": (128, 1, 4, 2), "h128b3": (128, 3, 20, 3), "h256b4": (256, 4, 20, 8)}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def energy(model, rows):
    """torch's own layers (F.mish, autograd-capable) in the dtype of the model: E [rows]."""
    F = torch.nn.functional
    lin_in, blocks, lin_out = model._parts()
    x = lin_in(rows)
    for l1, l2 in blocks:
        x = x + l2(F.mish(l1(F.mish(x))))
    return lin_out(x)[:, 0]


def langevin_step(model, st, x, coef, z, lo, hi, clip):
    """One update of langevin_mcmc.py:129-163 with torch.autograd.grad, in the dtype of the arguments."""
    with torch.enable_grad():
        xa = x.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad(energy(model, torch.cat([st, xa], dim=1)).sum(), xa)
    d = torch.minimum(torch.maximum(coef[0] * g + coef[1] * z, -clip), clip)
    return torch.minimum(torch.maximum(x - d, lo), hi)


class Case:
    """One problem: a random policy (weights of trained-like size: torch's initialisation times 1.6), scaled states, banks, and the chain in f64 and in
    torch f32 from the same banks."""

    def __init__(self, name, dev):
        from d3il_amd import policies as P
        self.dev = dev
        import copy
        hidden, nblk, obs, A = CASES[name]
        self.hidden, self.nblk, self.obs, self.A = hidden, nblk, obs, A
        self.pol = P.IBCPolicy.random(obs, A, device="cpu", seed=11, hidden_dim=hidden, n_blocks=nblk, weight_gain=1.6)
        rng = np.random.default_rng(hidden + nblk)
        p = self.pol
        p.lo, p.hi = torch.as_tensor(-1.2 - 0.3 * rng.random(A), dtype=torch.float32), torch.as_tensor(1.2 + 0.3 * rng.random(A), dtype=torch.float32)
        p.clip = (0.05 * (p.hi.double() - p.lo.double())).float()
        p.out_scale, p.out_shift = torch.as_tensor(0.004 * (1 + rng.random(A)), dtype=torch.float32), torch.as_tensor(0.001 * rng.normal(size=A), dtype=torch.float32)
        self.state = torch.as_tensor(rng.normal(size=(N, obs)), dtype=torch.float32)
        self.x0 = (p.lo + torch.as_tensor(rng.random((N, S, A)), dtype=torch.float32) * (p.hi - p.lo)).clamp(p.lo, p.hi)
        self.noise = torch.as_tensor(rng.normal(size=(K, N, S, A)), dtype=torch.float32)
        self.u = torch.as_tensor(rng.random(N), dtype=torch.float32)
        self.m64, self.m32 = copy.deepcopy(p.model).double().to(dev), copy.deepcopy(p.model).to(dev)      # (the chains run where the kernel runs: torch's own layers, autograd)
        self.packed = p._pack()
        # the chains: every iterate in f64, and torch's f32 chain
        self.xs64, self.e64 = self.chain(torch.float64)
        self.xs32, self.e32 = self.chain(torch.float32)
        pr = torch.softmax(-self.e64, dim=1)
        self.cdf64 = torch.cumsum(pr, dim=1)
        self.redrawn = 0
        for r in range(N):      # every row's pick is decided: a u within EDGE of an edge of the f64 CDF is drawn again
            while float((self.cdf64[r] - float(self.u[r])).abs().min()) < EDGE:
                self.u[r] = float(np.float32(int(rng.integers(0, 1 << 24)) / float(1 << 24))); self.redrawn += 1
        self.picks64 = self.pick_rule(self.e64, self.u)

    def rows(self, dt, n=N):
        return self.state[:n].to(self.dev, dt).unsqueeze(1).expand(n, S, self.obs).reshape(n * S, self.obs)

    def tables(self, dt):
        p = self.pol
        return tuple(v.to(self.dev, dt) for v in (p.coef, p.lo, p.hi, p.clip))

    def model(self, dt):
        return self.m64 if dt == torch.float64 else self.m32

    def chain(self, dt):
        model = self.model(dt)
        coef, lo, hi, clip = self.tables(dt)
        st, x = self.rows(dt), self.x0.to(self.dev, dt).reshape(N * S, self.A)
        xs = [x]
        for k in range(K):
            x = langevin_step(model, st, x, coef[k], self.noise[k].to(self.dev, dt).reshape(N * S, self.A) * self.pol.noise_scale, lo, hi, clip)
            xs.append(x)
        with torch.no_grad():
            e = energy(model, torch.cat([st, x], dim=1)).reshape(N, S)
        return [v.reshape(N, S, self.A).cpu() for v in xs], e.cpu()

    @staticmethod
    def pick_rule(e, u):
        """bin = min(#{s : c_s <= u S_sum}, S - 1) on prefix sums of exp(-(E_s - E_min)), in f64."""
        e = e.double()
        c = torch.cumsum(torch.exp(-(e - e.min(dim=1, keepdim=True).values)), dim=1)
        return (c <= u.double().unsqueeze(1) * c[:, -1:]).sum(dim=1).clamp_max(S - 1)


@functools.lru_cache(maxsize=None)
def _case(name, dev):
    return Case(name, dev)


def case(name, dev="cuda:0"):
    return _case(name, str(dev))


class Launch:
    """One call of d3il_ibc_langevin_f32 on device copies; results as host tensors.  Every pointer handed over is kept alive until the results are read."""

    def __init__(self, dev, c, n=N, k0=0, kk=K, x0="case", noise="case", u="case", state=None, seed=0, env_offset=0, t=0, t_dev=None, first=0, **shape):
        from d3il_amd import capi
        p, A = c.pol, c.A
        d = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float32).contiguous().to(dev)
        w = {k: d(v) for k, v in c.packed.items() if torch.is_tensor(v)}
        st = d(c.state[first:first + n] if state is None else state)
        x0 = d(c.x0[first:first + n] if isinstance(x0, str) else x0)
        nz = d(c.noise[k0:k0 + kk, first:first + n] if isinstance(noise, str) else noise)
        uu = d(c.u[first:first + n] if isinstance(u, str) else u)
        tabs = [d(p.coef[k0:k0 + kk]), d(p.lo), d(p.hi), d(p.clip), d(p.out_scale), d(p.out_shift)]
        self.t_dev = torch.tensor([t], dtype=torch.int32, device=dev) if t_dev is None else t_dev
        full = lambda *s, v=777.0, dtype=torch.float32: torch.full(s, v, dtype=dtype, device=dev)
        out = dict(actions=full(n, A), picks=full(n, v=99, dtype=torch.int32), x_final=full(n, S, A), energies=full(n, S), x0_out=full(n, S, A), noise_out=full(kk, n, S, A), u_out=full(n))
        ptr = lambda v: None if v is None else v.data_ptr()
        g = lambda key, default: shape.get(key, default)
        self.rc = capi.load().d3il_ibc_langevin_f32(ptr(st), ptr(w["w_in"]), ptr(w["b_in"]), ptr(w["w_blk"]), ptr(w["b_blk"]), ptr(w["w_out"]), ptr(w["b_out"]), ptr(w["wT_blk"]),
                                                    ptr(w["wT_act"]), ptr(tabs[0]), float(p.noise_scale), *(ptr(v) for v in tabs[1:]), int(seed), int(env_offset), ptr(self.t_dev),
                                                    ptr(x0), ptr(nz), ptr(uu), *(ptr(out[k]) for k in ("actions", "picks", "x_final", "energies", "x0_out", "noise_out", "u_out")),
                                                    n, g("obs", c.obs), g("A", A), g("hidden", c.hidden), g("nblk", c.nblk), g("S", S), g("K", kk), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        self.keep = (w, st, x0, nz, uu, tabs)
        self.dev_actions = out["actions"]
        for k, v in out.items():
            setattr(self, k, v.cpu())

    def bits(self):
        return [getattr(self, k).numpy().view(np.uint32 if k != "picks" else np.int32) for k in ("actions", "picks", "x_final", "energies", "x0_out", "noise_out", "u_out")]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("k", [0, 1, 9, 10, 19])
def test_one_teacher_forced_iteration(dev, name, k):
    """K = 1 from the f64 chain's iterate k (rounded to f32): the large first step, the schedule, its end, the two ends of the fixed-step loop.  The new x within
    4 x the deviation of torch's f32 autograd step from the f64 step on the same rows."""
    c = case(name)
    start = c.xs64[k].float()
    step = lambda dt: langevin_step(c.model(dt), c.rows(dt), start.to(c.dev, dt).reshape(N * S, c.A), c.tables(dt)[0][k], c.noise[k].to(c.dev, dt).reshape(N * S, c.A) * c.pol.noise_scale,
                                    *c.tables(dt)[1:]).reshape(N, S, c.A).cpu()
    want, t32 = step(torch.float64), step(torch.float32)
    yard = float((t32.double() - want).abs().max())
    out = Launch(dev, c, k0=k, kk=1, x0=start)
    err = float((out.x_final.double() - want).abs().max())
    print("%s k=%d: kernel %.3e, torch f32 %.3e (multiple %.2f)" % (name, k, err, yard, err / max(yard, 1e-30)))
    assert out.rc == 0 and torch.equal(out.x0_out, start) and torch.equal(out.noise_out[0], c.noise[k])
    assert err <= 4 * yard


@pytest.mark.parametrize("name", list(CASES))
def test_energies_and_picks_of_given_points(dev, name):
    """K = 0: the energies of the start points and the draw."""
    c = case(name)
    with torch.no_grad():
        rows = lambda dt: torch.cat([c.rows(dt), c.x0.to(c.dev, dt).reshape(N * S, c.A)], dim=1)
        e64, e32 = energy(c.m64, rows(torch.float64)).reshape(N, S).cpu(), energy(c.m32, rows(torch.float32)).reshape(N, S).cpu()
    cdf = torch.cumsum(torch.softmax(-e64, dim=1), dim=1)
    u = c.u.clone()
    rng = np.random.default_rng(5)
    for r in range(N):
        while float((cdf[r] - float(u[r])).abs().min()) < EDGE:
            u[r] = float(np.float32(int(rng.integers(0, 1 << 24)) / float(1 << 24)))
    out = Launch(dev, c, kk=0, u=u)
    yard, err = float((e32.double() - e64).abs().max()), float((out.energies.double() - e64).abs().max())
    print("%s K=0: energies kernel %.3e, torch f32 %.3e (multiple %.2f)" % (name, err, yard, err / yard))
    picks = Case.pick_rule(e64, u)
    assert out.rc == 0 and err <= 4 * yard and torch.equal(out.x_final, c.x0) and torch.equal(out.picks.long(), picks)
    want = c.x0[torch.arange(N), picks].double() * c.pol.out_scale.double() + c.pol.out_shift.double()
    assert float((out.actions.double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_the_whole_chain(dev, name):
    c = case(name)
    out = Launch(dev, c)
    yx, ye = float((c.xs32[-1].double() - c.xs64[-1]).abs().max()), float((c.e32.double() - c.e64).abs().max())
    ex, ee = float((out.x_final.double() - c.xs64[-1]).abs().max()), float((out.energies.double() - c.e64).abs().max())
    print("%s K=20: x kernel %.3e torch %.3e (multiple %.2f); E kernel %.3e torch %.3e (multiple %.2f); redrawn u %d of %d" % (name, ex, yx, ex / yx, ee, ye, ee / ye, c.redrawn, N))
    assert out.rc == 0 and ex <= 4 * yx and ee <= 4 * ye
    assert torch.equal(out.picks.long(), c.picks64)
    want = c.xs64[-1][torch.arange(N), c.picks64] * c.pol.out_scale.double() + c.pol.out_shift.double()
    assert float((out.actions.double() - want).abs().max()) <= 4 * yx * float(c.pol.out_scale.max()) + 4 * 2.0 ** -24 * float(want.abs().max())
    # clamp edges exact: whatever the bounds stopped sits on the bound bit for bit, and nothing lies outside
    lo, hi = c.pol.lo, c.pol.hi
    at = (c.xs64[-1] <= lo.double()) | (c.xs64[-1] >= hi.double())
    assert int(at.sum()) > 0 and bool(((out.x_final >= lo) & (out.x_final <= hi)).all())
    assert torch.equal(out.x_final[at], torch.where(c.xs64[-1] <= lo.double(), lo.expand(N, S, c.A), hi.expand(N, S, c.A))[at])


def test_a_clipped_step_moves_by_the_clip_exactly(dev):
    """The first step (0.5) of a steep network is stopped by the clip: x' = x -+ clip in f32 for those samples, computed as the kernel does (one subtraction)."""
    c = case("h128b3")
    out = Launch(dev, c, k0=0, kk=1)
    d64 = c.xs64[1] - c.xs64[0]
    clip = c.pol.clip
    inside = (c.xs64[0] - clip.double() > c.pol.lo.double() + 1e-6) & (c.xs64[0] + clip.double() < c.pol.hi.double() - 1e-6)
    stopped = (d64.abs() >= clip.double() * (1 - 1e-9)) & inside
    assert int(stopped.sum()) > 10
    want = torch.where(d64 < 0, c.x0 - clip, c.x0 + clip)
    assert torch.equal(out.x_final[stopped], want[stopped])


@pytest.mark.parametrize("name", ["h128b1", "h256b4"])
def test_rows_do_not_depend_on_the_launch(dev, name):
    c = case(name)
    whole = Launch(dev, c).bits()
    for n in (1, 3, 16):
        part = Launch(dev, c, n=n).bits()
        for a, b in zip(part, whole):
            assert np.array_equal(a, b[:, :n] if a.ndim == 4 else b[:n]), n
    # with Philox: env_offset 5, n_env 4 = rows 5 .. 8 of env_offset 0, n_env 17
    w = Launch(dev, c, x0=None, noise=None, u=None, seed=77, t=3).bits()
    p = Launch(dev, c, n=4, first=5, x0=None, noise=None, u=None, seed=77, t=3, env_offset=5).bits()
    for a, b in zip(p, w):
        assert np.array_equal(a, b[:, 5:9] if a.ndim == 4 else b[5:9])


def test_philox_stream(dev):
    from d3il_amd import policies as P
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    seed, t = 0x1234567890ABCDEF, 7
    for name in ("h128b1", "h256b4"):      # A = 2: one call per sample; A = 8: two
        c = case(name)
        out = Launch(dev, c, x0=None, noise=None, u=None, seed=seed, t=t)
        u0 = torch.as_tensor(P.ibc_start_uniforms(seed, 0, N, t, c.A))
        assert torch.equal(out.x0_out, c.pol.lo + u0 * (c.pol.hi - c.pol.lo))      # uniforms exactly, the start point in f32 operation by operation
        assert torch.equal(out.u_out, torch.as_tensor(P.ibc_pick_uniforms(seed, 0, N, t)))
        for k in (0, 7, K - 1):
            want = P.ibc_normals(seed, 0, N, t, k, c.A)
            r = torch.as_tensor(P.ibc_words(seed, 0, N, t, 1, k).astype(np.int64))
            u1, u2 = ((r[..., 0::2] >> 8) + 1).float() * 2.0 ** -24, (r[..., 1::2] >> 8).float() * 2.0 ** -24      # [N, S, q, pair]
            rad, ang = torch.sqrt(-2.0 * torch.log(u1)), 6.28318530717958647692 * u2
            t32 = torch.stack((rad * torch.cos(ang), rad * torch.sin(ang)), dim=-1).reshape(N, S, 8)[:, :, :c.A]
            yard = float(np.abs(t32.double().numpy() - want).max())
            err = float(np.abs(out.noise_out[k].double().numpy() - want).max())
            print("%s normals k=%d: kernel %.3e torch f32 %.3e" % (name, k, err, yard))
            assert err <= 4 * yard
        assert not torch.equal(out.noise_out[0], out.noise_out[1])
    c = case("h128b1")
    out = Launch(dev, c, x0=None, noise=None, u=None, seed=seed, t=t)
    # other words than d3il_policy_action's (fourth word 0), the BeT head's and the DDPM-GPT step's for the same (seed, env, t)
    env = ObstacleAvoidanceVecEnv(64, device=0)
    try:
        env.start(); env.reset(); env.policy_begin()
        tcp = env.robot_state().clone()
        act = torch.zeros(64, 7, dtype=torch.float64, device=env.device)
        env.policy_action(seed, 0, t, act)
        torch.cuda.synchronize()
        u_harness = ((act[:, 0] - tcp[:, 0] + 0.01) / 0.02).cpu().numpy()[:N]
    finally:
        env.close()
    mine = np.concatenate([P.ibc_words(seed, 0, N, t, kind, k).reshape(N, -1) for kind, k in ((0, 0), (1, 0), (1, 19), (2, 0))], axis=1)
    others = np.concatenate([np.stack(P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, np.arange(N), 0, t, tag), axis=-1) for tag in (0, P.BET_TAG)]
                            + [P.ddpm_gpt_words(seed, 0, N, t, k, 16).reshape(N, -1) for k in (1, 8, 255)], axis=1)
    assert not np.isin(mine, others).any()
    pick_u = out.u_out.numpy().astype(np.float64)
    assert float(np.abs(u_harness - pick_u).min()) > 2.0 ** -20 and float(np.abs(P.bet_uniforms(seed, 0, N, t).astype(np.float64) - pick_u).min()) > 2.0 ** -20
    # the device step word: the same word -> the same bits, advanced -> other draws
    word = torch.tensor([t], dtype=torch.int32, device=dev)
    a = Launch(dev, c, x0=None, noise=None, u=None, seed=seed, t_dev=word)
    b = Launch(dev, c, x0=None, noise=None, u=None, seed=seed, t_dev=word)
    word.add_(1)
    d = Launch(dev, c, x0=None, noise=None, u=None, seed=seed, t_dev=word)
    for x, y, z in zip(a.bits(), b.bits(), out.bits()):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert not torch.equal(d.x0_out, a.x0_out) and not torch.equal(d.noise_out, a.noise_out) and not torch.equal(d.u_out, a.u_out)
    assert torch.equal(d.u_out, torch.as_tensor(P.ibc_pick_uniforms(seed, 0, N, t + 1)))


def test_nonfinite_inputs_mark_their_environment_only(dev):
    c = case("h128b3")
    clean = Launch(dev, c)
    assert (clean.picks >= 0).all() and torch.isfinite(clean.actions).all()
    state, x0 = c.state.clone(), c.x0.clone()
    state[3, 7], state[9, 0] = float("nan"), float("inf")
    x0[12, 37, 1] = float("nan")
    bad = Launch(dev, c, state=state, x0=x0)
    hit = [3, 9, 12]
    good = [r for r in range(N) if r not in hit]
    assert bad.picks[hit].tolist() == [-1, -1, -1] and torch.isnan(bad.actions[hit]).all()
    for a, b in zip(bad.bits(), clean.bits()):
        assert np.array_equal(a[:, good] if a.ndim == 4 else a[good], b[:, good] if b.ndim == 4 else b[good])


def test_a_nan_environment_raises_solver_fail_in_its_avoiding_lane_only(dev):
    """The kernel's NaN action, used as Avoiding_Sim uses a policy output (desired xy = action + previous desired xy), for one env step."""
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    c = case("h128b1")
    n = 6
    state = c.state[:n].clone()
    state[2, 1] = float("nan")
    out = Launch(dev, c, n=n, state=state)
    assert out.picks[2] == -1 and (np.delete(out.picks.numpy(), 2) >= 0).all()
    env = ObstacleAvoidanceVecEnv(n, device=0)
    try:
        env.start(); env.reset()
        rs = env.robot_state().clone()
        quat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=env.device).expand(n, 4)
        env.step(torch.cat((rs[:, :2] + out.dev_actions.to(torch.float64), rs[:, 2:3], quat), dim=1).contiguous())
        torch.cuda.synchronize()
        fail = (env.flags[:n] & SOLVER_FAIL) != 0
        assert fail.tolist() == [r == 2 for r in range(n)]
    finally:
        env.close()


def test_unsupported_shapes_are_refused_before_any_launch(dev):
    c = case("h128b1")
    for kw in (dict(hidden=64), dict(S=32), dict(A=9), dict(obs=27), dict(K=64), dict(nblk=5)):      # (obs 27 + A 2 = 29; five blocks: one more than the derivative register sets)
        o = Launch(dev, c, n=4, **kw)
        assert o.rc == -5, kw
        assert (o.picks == 99).all() and all(bool((getattr(o, k) == 777.0).all()) for k in ("actions", "x_final", "energies", "x0_out", "noise_out", "u_out")), kw
    ok = Launch(dev, c, n=4)
    assert ok.rc == 0 and (ok.picks >= 0).all() and (ok.picks <= 63).all()


def test_five_blocks_take_the_torch_chain(dev, monkeypatch):
    """More residual blocks than the kernel keeps derivative sets for: the policy does not call the entry (which would refuse) but runs the torch chain, on the device."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_IBC_FUSED", raising=False)
    pol = P.IBCPolicy.random(4, 2, device=dev, seed=2, hidden_dim=128, n_blocks=5, policy_seed=3)
    obs = torch.randn(3, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    assert not pol.fused_ok(obs)
    with pytest.warns(UserWarning, match="torch chain"):
        y = pol.predict_batch(obs)
    assert y.shape == (3, 2) and torch.isfinite(y).all() and pol._packed.key is None and (pol.last_picks >= 0).all()
    assert np.array_equal(pol.last_u.cpu().numpy(), P.ibc_pick_uniforms(3, 0, 3, 0))
