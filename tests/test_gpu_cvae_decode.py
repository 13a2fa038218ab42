"""d3il_cvae_decode_f32 (csrc/policy_cvae.h) on the GPU against an f64 torch restatement, the latent given (z_in) or drawn (Philox): 17 environments = one full
16-row tile and a tail of one.  The yardstick of every accuracy assertion is the deviation of torch's own f32 layers on the same rows from the f64 result."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 17
SOLVER_FAIL = 1 << 16
# name: (hidden, residual blocks, obs, latent, action components)
CASES = {"h128b0": (128, 0, 4, 32, 2), "h128b1": (128, 1, 20, 16, 8), "h128b3": (128, 3, 22, 24, 2), "h256b4": (256, 4, 32, 32, 16)}
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class Case:
    """A random-weight policy (outputs of a few tenths against bounds of +-0.3: some reach the clamp), scaled states, an unclamped latent bank, and - computed once -
    the f64 result and torch's f32 result on the same rows (both on the host)."""

    def __init__(self, name):
        from d3il_amd import policies as P
        self.hidden, self.nblk, self.obs, self.L, self.A = CASES[name]
        i = list(CASES).index(name)
        self.pol = P.CVAEPolicy.random(self.obs, self.A, device="cpu", seed=40 + i, hidden_dim=self.hidden, n_blocks=self.nblk, latent_dim=self.L, weight_gain=1.6,
                                       action_scale=0.004, bound=0.3)
        self.pol.out_shift = (torch.arange(self.A, dtype=torch.float32) * 0.001 - 0.003).contiguous()      # a shift, so that the inverse scaling is a product AND a sum
        g = torch.Generator().manual_seed(50 + i)
        self.state = torch.randn(N, self.obs, generator=g) * 0.8
        self.z = torch.randn(N, self.L, generator=g)
        m64 = copy.copy(self.pol)
        m64.model = copy.deepcopy(self.pol.model).double()
        self.pol64 = m64
        self.want, self.zc = m64._decode_torch(self.state.double(), self.z.double())
        self.t32, _ = self.pol._decode_torch(self.state, self.z)
        self.yard = float((self.t32.double() - self.want).abs().max())
        self.pk = None

    def packed(self, dev):
        if self.pk is None:
            self.pk = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in self.pol._pack().items()}
        return self.pk


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


class Launch:
    """One call of the entry point.  ``z``: "bank" = the case's z_in, None = Philox, or a tensor.  Outputs are poisoned with 777 before the call."""

    def __init__(self, dev, c, n=N, first=0, state=None, z="bank", seed=0, t=0, t_dev=None, env_offset=0, z_out=True, **over):
        from d3il_amd import capi
        pk = c.packed(dev)
        st = (c.state if state is None else state)[first:first + n].to(dev).contiguous()
        zt = c.z if isinstance(z, str) else z
        zt = None if zt is None else zt[first:first + n].to(dev).contiguous()
        hidden, L, obs, A, nblk = (over.get(k, d) for k, d in (("hidden", c.hidden), ("L", c.L), ("obs", c.obs), ("A", c.A), ("nblk", c.nblk)))
        word = t_dev if t_dev is not None else torch.tensor([t], dtype=torch.int32, device=dev)
        f = lambda v: v.to(dev).contiguous()
        self.keep = (f(c.pol.lo), f(c.pol.hi), f(c.pol.out_scale), f(c.pol.out_shift), st, zt, word)
        lo, hi, sc, sh = self.keep[:4]
        act = torch.full((n, max(A, 1)), 777.0, device=dev)
        zo = torch.full((n, c.L), 777.0, device=dev)
        self.rc = capi.load().d3il_cvae_decode_f32(st.data_ptr(), pk["w_in"].data_ptr(), pk["b_in"].data_ptr(), pk["w_blk"].data_ptr(), pk["b_blk"].data_ptr(), pk["w_out"].data_ptr(),
                                                   pk["b_out"].data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(), sh.data_ptr(), seed, env_offset, word.data_ptr(),
                                                   None if zt is None else zt.data_ptr(), act.data_ptr(), zo.data_ptr() if z_out else None, n, obs, L, A, hidden, nblk,
                                                   torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        self.dev_actions = act
        self.actions, self.z_out = act.cpu(), zo.cpu()

    def bits(self):
        return self.actions.numpy().view(np.uint32), self.z_out.numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_actions_against_f64(dev, name):
    c = case(name)
    out = Launch(dev, c)
    assert out.rc == 0
    lo, hi = c.pol.lo.double(), c.pol.hi.double()
    raw = torch.cat([c.state.double(), c.zc], dim=1)
    for layer in c.pol64.model.layers:
        raw = layer(raw)
    clamped = int(((raw < lo) | (raw > hi)).sum())
    assert 0 < clamped < raw.numel()      # both sides of the action clamp
    err = float((out.actions.double() - c.want).abs().max())
    print("%s: kernel %.3e, torch f32 %.3e -> %.2f yardsticks (%d of %d outputs clamped; largest action %.3e)" % (name, err, c.yard, err / c.yard, clamped, raw.numel(), float(c.want.abs().max())))
    assert c.yard > 0 and err <= 4 * c.yard
    assert torch.equal(out.z_out, c.z.clamp(-0.5, 0.5))      # the clamped latent that was used, bit for bit
    assert 0.4 < float((out.z_out.abs() == 0.5).float().mean()) < 0.8
    # without z_out: the same actions
    assert np.array_equal(Launch(dev, c, z_out=False).bits()[0], out.bits()[0])


def test_clamp_edges_are_exact(dev):
    """Outputs driven past both bounds come out as inverse_scale(bound) bit for bit (f64 product and sum of the f32 operands, rounded once); latents beyond +-0.5
    come out as +-0.5, latents inside unchanged."""
    c = copy.copy(case("h128b1"))
    c.pol = copy.copy(c.pol)
    c.pol.model = copy.deepcopy(c.pol.model)
    c.pk = None
    with torch.no_grad():
        c.pol.model.layers[-1].bias.copy_(torch.tensor([100.0, -100.0] * (c.A // 2)))
    z = c.z.clone()
    z[:, 0], z[:, 1], z[:, 2], z[:, 3] = 0.5000001, -0.5000001, 7.0, -3e30
    z[:, 4], z[:, 5] = 0.49999997, -0.25
    out = Launch(dev, c, z=z)
    p = c.pol
    want_hi = (p.hi.double() * p.out_scale.double() + p.out_shift.double()).float()
    want_lo = (p.lo.double() * p.out_scale.double() + p.out_shift.double()).float()
    want = torch.where(torch.arange(c.A) % 2 == 0, want_hi, want_lo).expand(N, c.A)
    assert np.array_equal(out.actions.numpy().view(np.uint32), want.contiguous().numpy().view(np.uint32))
    zo = out.z_out
    assert (zo[:, 0] == 0.5).all() and (zo[:, 1] == -0.5).all() and (zo[:, 2] == 0.5).all() and (zo[:, 3] == -0.5).all()
    assert torch.equal(zo[:, 4:6], z[:, 4:6]) and torch.equal(zo, z.clamp(-0.5, 0.5))


@pytest.mark.parametrize("name", ["h128b1", "h256b4"])
def test_rows_do_not_depend_on_the_launch(dev, name):
    c = case(name)
    whole = Launch(dev, c).bits()
    for n in (1, 3, 16):
        for a, b in zip(Launch(dev, c, n=n).bits(), whole):
            assert np.array_equal(a, b[:n]), n
    # with Philox: launches of 1, 3 and 16 environments, and env_offset 5, n_env 4 = rows 5 .. 8 of env_offset 0, n_env 17
    w = Launch(dev, c, z=None, seed=77, t=3).bits()
    for n in (1, 3, 16):
        for a, b in zip(Launch(dev, c, n=n, z=None, seed=77, t=3).bits(), w):
            assert np.array_equal(a, b[:n]), n
    p = Launch(dev, c, n=4, first=5, z=None, seed=77, t=3, env_offset=5).bits()
    for a, b in zip(p, w):
        assert np.array_equal(a, b[5:9])
    assert not np.array_equal(w[1][0], w[1][1])


def test_philox_stream(dev):
    from d3il_amd import policies as P
    seed, t = 0x1234567890ABCDEF, 7
    for name in ("h128b0", "h128b1", "h128b3"):      # latents of 32, 16 and 24: eight, four and six calls per row
        c = case(name)
        out = Launch(dev, c, z=None, seed=seed, t=t)
        want = np.clip(P.cvae_latent_normals(seed, 0, N, t, c.L), -0.5, 0.5)
        r = torch.as_tensor(P.cvae_words(seed, 0, N, t).astype(np.int64))
        u1, u2 = ((r[..., 0::2] >> 8) + 1).float() * 2.0 ** -24, (r[..., 1::2] >> 8).float() * 2.0 ** -24      # [N, q, pair]
        rad, ang = torch.sqrt(-2.0 * torch.log(u1)), 6.28318530717958647692 * u2
        t32 = torch.stack((rad * torch.cos(ang), rad * torch.sin(ang)), dim=-1).reshape(N, 32)[:, :c.L].clamp(-0.5, 0.5)
        yard = float(np.abs(t32.double().numpy() - want).max())
        err = float(np.abs(out.z_out.double().numpy() - want).max())
        moved = float((out.z_out.abs() == 0.5).float().mean())
        print("%s latent: kernel %.3e torch f32 %.3e -> %.2f yardsticks; on a bound %.3f" % (name, err, yard, err / yard, moved))
        assert yard > 0 and err <= 4 * yard
        # the actions are the decoder's on that latent: the same launch with z_out handed back as z_in
        again = Launch(dev, c, z=out.z_out)
        assert np.array_equal(again.bits()[0], out.bits()[0])
    # other words than d3il_policy_action's (fourth word 0), the BeT head's, the DDPM-GPT step's, the IBC chain's and the ACT chunk's for the same (seed, env, t)
    mine = P.cvae_words(seed, 0, N, t).reshape(N, -1)
    others = np.concatenate([np.stack(P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, np.arange(N), 0, t, tag), axis=-1) for tag in (0, P.BET_TAG)]
                            + [P.ddpm_gpt_words(seed, 0, N, t, k, 16).reshape(N, -1) for k in (1, 8, 255)]
                            + [P.ibc_words(seed, 0, N, t, kind, k).reshape(N, -1) for kind, k in ((0, 0), (1, 0), (1, 19), (2, 0))]
                            + [P.act_latent_words(seed, 0, N, t).reshape(N, -1)], axis=1)
    assert not np.isin(mine, others).any()
    # the device step word: the same word -> the same bits, advanced -> the draws of t + 1
    c = case("h128b1")
    out = Launch(dev, c, z=None, seed=seed, t=t)
    word = torch.tensor([t], dtype=torch.int32, device=dev)
    a = Launch(dev, c, z=None, seed=seed, t_dev=word)
    b = Launch(dev, c, z=None, seed=seed, t_dev=word)
    word.add_(1)
    d = Launch(dev, c, z=None, seed=seed, t_dev=word)
    e = Launch(dev, c, z=None, seed=seed, t=t + 1)
    for x, y, z in zip(a.bits(), b.bits(), out.bits()):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert not torch.equal(d.z_out, a.z_out) and not torch.equal(d.actions, a.actions)
    for x, y in zip(d.bits(), e.bits()):
        assert np.array_equal(x, y)
    # seed and offset reach the counter
    assert not torch.equal(Launch(dev, c, z=None, seed=seed + 1, t=t).z_out, out.z_out)
    far = Launch(dev, c, z=None, seed=seed, t=t, env_offset=(1 << 32) + 2, n=4).z_out      # the high counter word
    assert float(np.abs(far.double().numpy() - np.clip(P.cvae_latent_normals(seed, (1 << 32) + 2, 4, t, c.L), -0.5, 0.5)).max()) < 1e-5
    assert not torch.equal(far, Launch(dev, c, z=None, seed=seed, t=t, env_offset=2, n=4).z_out)


@pytest.mark.parametrize("name", ["h128b3", "h256b4"])
def test_nonfinite_inputs_mark_their_environment_only(dev, name):
    c = case(name)
    clean = Launch(dev, c)
    assert torch.isfinite(clean.actions).all()
    state, z = c.state.clone(), c.z.clone()
    state[3, c.obs - 1], state[9, 0] = float("nan"), float("inf")
    z[12, c.L - 1] = float("nan")
    z[16, 0] = float("-inf")      # (the tail row of the second workgroup)
    bad = Launch(dev, c, state=state, z=z)
    hit = [3, 9, 12, 16]
    good = [r for r in range(N) if r not in hit]
    assert torch.isnan(bad.actions[hit]).all()
    assert np.array_equal(bad.actions[hit].numpy().view(np.uint32), np.full((4, c.A), 0x7FC00000, dtype=np.uint32))
    for a, b in zip(bad.bits(), clean.bits()):
        assert np.array_equal(a[good], b[good])
    assert torch.isnan(bad.z_out[12, c.L - 1]) and torch.isnan(bad.z_out[16, 0]) and torch.equal(bad.z_out[[3, 9]], clean.z_out[[3, 9]])


def test_a_nonfinite_output_marks_its_environment(dev):
    """A decoder output beyond the f32 range (an Inf the action clamp would turn into a bound) gives NaN: one row's state drives the sum over the edge."""
    c = copy.copy(case("h128b0"))
    c.pol = copy.copy(c.pol)
    c.pol.model = copy.deepcopy(c.pol.model)
    c.pk = None
    with torch.no_grad():
        c.pol.model.layers[-1].weight.mul_(1e4)
    clean = Launch(dev, c)
    state = c.state.clone()
    state[5] = 3e37
    out = Launch(dev, c, state=state)
    good = [r for r in range(N) if r != 5]
    assert torch.isnan(out.actions[5]).all() and np.array_equal(out.bits()[0][good], clean.bits()[0][good])


def test_a_nan_environment_raises_solver_fail_in_its_avoiding_lane_only(dev):
    """The kernel's NaN action, used as Avoiding_Sim uses a policy output (desired xy = action + previous desired xy), for one env step."""
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    c = case("h128b0")      # obs 4 -> 2 actions: Avoiding's shape
    n = 6
    state = c.state[:n].clone()
    state[2, 1] = float("nan")
    out = Launch(dev, c, n=n, state=state)
    assert torch.isnan(out.actions[2]).all() and torch.isfinite(out.actions[[0, 1, 3, 4, 5]]).all()
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
    for kw in (dict(hidden=64), dict(L=33), dict(obs=49, L=16), dict(obs=33, L=32), dict(A=17), dict(obs=0), dict(L=0), dict(A=0)):      # (49 + 16 = 33 + 32 = 65 inputs)
        o = Launch(dev, c, n=4, **kw)
        assert o.rc == -5, kw
        assert bool((o.actions == 777.0).all()) and bool((o.z_out == 777.0).all()), kw
    from d3il_amd import capi
    assert b"d3il_cvae_decode_f32" in capi.load().d3il_last_error()
    ok = Launch(dev, c, n=4)
    assert ok.rc == 0 and torch.isfinite(ok.actions).all() and not bool((ok.actions == 777.0).any())
    assert Launch(dev, c, n=4, nblk=-1).rc == -5


def test_an_unsupported_decoder_takes_torchs_layers(dev, monkeypatch):
    """A hidden width the kernel is not built for: the policy does not call the entry (which would refuse) but runs torch's layers, on the device, and says so once."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_CVAE_FUSED", raising=False)
    pol = P.CVAEPolicy.random(4, 2, device=dev, seed=2, hidden_dim=64, n_blocks=1, latent_dim=16, policy_seed=3)
    obs = torch.randn(3, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    assert not pol.fused_ok(obs)
    with pytest.warns(UserWarning, match="torch's layers"):
        y = pol.predict_batch(obs)
    assert y.shape == (3, 2) and torch.isfinite(y).all() and pol._packed.key is None
    assert np.array_equal(pol.last_z.cpu().numpy(), np.clip(P.cvae_latent_normals(3, 0, 3, 0, 16).astype(np.float32), np.float32(-0.5), np.float32(0.5)))
