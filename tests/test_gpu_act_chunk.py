"""k_act_chunk (csrc/policy_act.h) through d3il_act_chunk_f32 on the GPU against an f64 torch restatement (policies.ACTPolicy._chunk_torch on a double copy of the
network), all banks given unless the test is about Philox.

Geometry: one workgroup of four waves per 16 environments; 17 environments = one full tile and a tail tile of one.  Shapes: (obs, A, T, encoder layers, decoder
layers) = (4, 2, 1, 1, 1) - T = 1: one position row for both encoder tokens, no mask -, (10, 2, 3, 2, 4) - the shipped one - and (20, 8, 8, 2, 4) - every token
register, both action lanes groups, two input tiles.  The yardstick of a case is the deviation of torch's own f32 evaluation of that case (its own layers, on the
same device) from the f64 one, taken per case and never carried over; the bar is 4 of them."""
import copy
import functools
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SOLVER_FAIL = 1 << 16
N = 17
CASES = {"t1": (4, 2, 1, 1, 1), "shipped": (10, 2, 3, 2, 4), "t8": (20, 8, 8, 2, 4)}
POISON = 777.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(name):
    """Network, inputs and the f64 reference of a case (computed once, shared, never modified)."""
    from d3il_amd import policies as P
    obs, A, T, enc, dec = CASES[name]
    pol = P.ACTPolicy.random(obs, A, T, device="cpu", seed=11, enc_layers=enc, dec_layers=dec, policy_seed=23, bound=3.5)      # (heads of order 3: a minority of entries on a bound)
    g = torch.Generator().manual_seed(7)
    state = torch.randn(N, obs, generator=g) * 0.7
    latent = torch.rand(N, 32, generator=g)
    prior = torch.randn(N, T, A, generator=g) * 0.002      # what the lanes that are not due emit from
    p64 = copy.copy(pol)
    p64.model = copy.deepcopy(pol.model).double()
    ref64 = p64._chunk_torch(state.double(), latent.double())
    head64 = p64.model(state.double(), latent.double())
    return types.SimpleNamespace(name=name, obs=obs, A=A, T=T, enc=enc, dec=dec, pol=pol, state=state, latent=latent, prior=prior, ref64=ref64, head64=head64, pk=pol._pack())


class Launch:
    """One call of the entry point on the first n rows of a case.  ``counter`` / ``chunk``: the persistent state before the call (default: every lane due, chunk
    poisoned); ``latent``: "bank" (the case's), None (Philox) or a tensor."""

    def __init__(self, dev, c, n=N, state=None, latent="bank", counter=None, chunk=None, env_offset=0, seed=23, t=0, rows=None, **over):
        from d3il_amd import capi
        rows = slice(0, n) if rows is None else rows
        f = lambda v: v.to(dev).contiguous()
        pk = {k: f(v) for k, v in c.pk.items()}
        pol = c.pol
        st = f((c.state if state is None else state)[rows].clone())
        z = f(c.latent[rows].clone()) if isinstance(latent, str) else (None if latent is None else f(latent))
        cnt = f(torch.full((n,), c.T, dtype=torch.int32) if counter is None else torch.as_tensor(counter, dtype=torch.int32))
        ch = f(torch.full((n, c.T, c.A), POISON) if chunk is None else chunk.clone())
        act, lat_out = torch.full((n, c.A), POISON, device=dev), torch.full((n, 32), POISON, device=dev)
        tw = torch.tensor([t], dtype=torch.int32, device=dev)
        lo, hi, sc, sh = f(pol.lo), f(pol.hi), f(pol.out_scale), f(pol.out_shift)
        a = dict(obs=c.obs, A=c.A, T=c.T, width=64, heads=4, latent=32, enc=c.enc, dec=c.dec)
        a.update(over)
        self.rc = capi.load().d3il_act_chunk_f32(st.data_ptr(), pk["w_in"].data_ptr(), pk["tab"].data_ptr(), pk["enc_w"].data_ptr(), pk["enc_v"].data_ptr(), pk["dec_w"].data_ptr(),
                                                 pk["dec_v"].data_ptr(), pk["head_w"].data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(),
                                                 sh.data_ptr(), seed, env_offset, tw.data_ptr(), None if z is None else z.data_ptr(), cnt.data_ptr(), ch.data_ptr(),
                                                 act.data_ptr(), lat_out.data_ptr(), n, a["obs"], a["A"], a["T"], a["width"], a["heads"], a["latent"], a["enc"], a["dec"],
                                                 torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        self.dev_actions = act
        self.actions, self.counter, self.chunk, self.latent_out, self.t_word = act.cpu(), cnt.cpu(), ch.cpu(), lat_out.cpu(), int(tw.item())

    def bits(self):
        return [v.numpy().view(np.uint32) if v.dtype == torch.float32 else v.numpy() for v in (self.actions, self.counter, self.chunk, self.latent_out)]


@pytest.mark.parametrize("name", list(CASES))
def test_chunks_within_four_yardsticks_of_f64_and_clamp_edges_exact(dev, name):
    c = case(name)
    pol = c.pol
    p32 = copy.copy(pol)
    p32.model = copy.deepcopy(pol.model).to(dev)
    for k in ("lo", "hi", "out_scale", "out_shift"):
        setattr(p32, k, getattr(pol, k).to(dev))
    yard = float((p32._chunk_torch(c.state.to(dev), c.latent.to(dev)).cpu().double() - c.ref64).abs().max())
    o = Launch(dev, c)
    assert o.rc == 0
    err = float((o.chunk.double() - c.ref64).abs().max())
    print("%s: kernel %.3e, torch f32 %.3e: %.2f yardsticks (chunk magnitude %.3e)" % (name, err, yard, err / yard, float(c.ref64.abs().max())))
    assert err <= 4 * yard
    lo, hi = pol.lo.double(), pol.hi.double()
    below, above = c.head64 < lo - 1e-4, c.head64 > hi + 1e-4      # decided clamps: the head's f64 value is clearly outside
    e_lo, e_hi = (pol.lo * pol.out_scale + pol.out_shift).expand_as(o.chunk), (pol.hi * pol.out_scale + pol.out_shift).expand_as(o.chunk)
    assert int(below.sum() + above.sum()) > 0 and int((~below & ~above).sum()) > int(below.sum() + above.sum())
    assert torch.equal(o.chunk[below], e_lo[below]) and torch.equal(o.chunk[above], e_hi[above])
    assert torch.equal(o.actions, o.chunk[:, 0]) and o.counter.tolist() == [1] * N and torch.equal(o.latent_out, c.latent) and o.t_word == 0


def _flip(p, T):      # another phase: a due lane waits, a waiting lane is due
    return 0 if p == T else T


@pytest.mark.parametrize("name", list(CASES))
def test_a_lane_does_not_depend_on_the_phase_of_its_tile_mates(dev, name):
    c = case(name)
    T = c.T
    mixed = [(T, *range(T))[i % (T + 1)] for i in range(N)]      # due, 0, 1, .., T - 1, due, ..
    X = Launch(dev, c, counter=mixed, chunk=c.prior)
    due = torch.tensor([p == T for p in mixed])
    assert bool(due[:16].any()) and bool((~due[:16]).any())
    # lanes that are not due: their chunk and latent are untouched, they emit the stored row
    assert np.array_equal(X.chunk[~due].numpy().view(np.uint32), c.prior[~due].numpy().view(np.uint32)) and bool((X.latent_out[~due] == POISON).all())
    for i in range(N):
        want = X.chunk[i, 0] if mixed[i] == T else c.prior[i, mixed[i]]
        assert torch.equal(X.actions[i], want) and int(X.counter[i]) == (1 if mixed[i] == T else mixed[i] + 1)
    assert torch.equal(X.latent_out[due], c.latent[due])
    for keep in (0, 1):      # the lanes of one parity keep their phase, their tile-mates take another one
        other = [p if i % 2 == keep else _flip(p, T) for i, p in enumerate(mixed)]
        Y = Launch(dev, c, counter=other, chunk=c.prior)
        sel = torch.arange(N) % 2 == keep
        for a, b in zip(X.bits(), Y.bits()):
            assert np.array_equal(a[sel.numpy()], b[sel.numpy()])
    # and equal to the launch in which every lane is due
    full = Launch(dev, c, chunk=c.prior)
    assert np.array_equal(X.chunk[due].numpy().view(np.uint32), full.chunk[due].numpy().view(np.uint32))
    # no lane due: only actions and counters are written, the state rows are not read
    waiting = [i % T for i in range(N)]
    Z = Launch(dev, c, counter=waiting, chunk=c.prior, state=torch.full_like(c.state, float("nan")))
    assert np.array_equal(Z.chunk.numpy().view(np.uint32), c.prior.numpy().view(np.uint32)) and bool((Z.latent_out == POISON).all())
    assert torch.equal(Z.actions, c.prior[torch.arange(N), torch.tensor(waiting)]) and Z.counter.tolist() == [w + 1 for w in waiting]


def test_rows_do_not_depend_on_the_launch_and_latents_are_the_host_philox(dev):
    from d3il_amd import policies as P
    c = case("shipped")
    seed, t = 0x1234567890ABCDEF, 7
    whole = Launch(dev, c, latent=None, seed=seed, t=t)
    assert np.array_equal(whole.latent_out.numpy(), P.act_latent_uniforms(seed, 0, N, t)) and whole.t_word == t      # (the kernel reads the step word; its owner advances it)
    for n in (1, 3, 16):
        part = Launch(dev, c, n=n, latent=None, seed=seed, t=t)
        for a, b in zip(whole.bits(), part.bits()):
            assert np.array_equal(a[:n], b), n
    off = Launch(dev, c, n=4, rows=slice(5, 9), latent=None, seed=seed, t=t, env_offset=5)
    for a, b in zip(whole.bits(), off.bits()):
        assert np.array_equal(a[5:9], b)
    assert np.array_equal(Launch(dev, c, n=2, latent=None, seed=seed, t=t, env_offset=(1 << 32) - 1).latent_out.numpy(), P.act_latent_uniforms(seed, (1 << 32) - 1, 2, t))
    moved = Launch(dev, c, latent=None, seed=seed, t=t + 1)
    assert not np.isin(moved.latent_out.numpy(), whole.latent_out.numpy()).all()


def test_the_step_word_advances_once_per_call(dev, monkeypatch):
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_ACT_FUSED", raising=False)
    pol = P.ACTPolicy.random(4, 2, 1, device=dev, seed=11, enc_layers=1, dec_layers=1, policy_seed=5)      # T = 1: every call draws
    obs = case("t1").state.to(dev)
    for t in range(3):
        assert pol.fused_ok(obs)
        pol.predict_batch(obs)
        assert int(pol._t) == t + 1 and np.array_equal(pol.last_latent.cpu().numpy(), P.act_latent_uniforms(5, 0, N, t))


@pytest.mark.parametrize("name", ["shipped", "t8"])
def test_nonfinite_state_marks_its_lane_only(dev, name):
    c = case(name)
    clean = Launch(dev, c, chunk=c.prior)
    state = c.state.clone()
    state[3, 1], state[16, c.obs - 1] = float("nan"), float("inf")      # (lane 16: the tail tile)
    bad = Launch(dev, c, state=state, chunk=c.prior)
    hit = [3, 16]
    good = [r for r in range(N) if r not in hit]
    assert torch.isnan(bad.chunk[hit]).all() and torch.isnan(bad.actions[hit]).all() and bad.counter.tolist() == [1] * N
    for a, b in zip(bad.bits(), clean.bits()):
        assert np.array_equal(a[good], b[good])
    # a NaN in the state row of a lane that is not due changes nothing
    cnt = [c.T if i % 2 == 0 else 0 for i in range(N)]
    base = Launch(dev, c, counter=cnt, chunk=c.prior)
    state = c.state.clone()
    state[5, 0] = float("nan")
    same = Launch(dev, c, counter=cnt, chunk=c.prior, state=state)
    for a, b in zip(base.bits(), same.bits()):
        assert np.array_equal(a, b)


def test_a_nan_lane_raises_solver_fail_in_its_avoiding_lane_only(dev):
    """The kernel's NaN action, used as Avoiding_Sim uses a policy output (desired xy = action + previous desired xy), for one env step."""
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    c = case("t1")
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
    c = case("shipped")
    for kw in (dict(width=128), dict(heads=8), dict(T=9), dict(A=9), dict(obs=33), dict(enc=5), dict(dec=9)):
        o = Launch(dev, c, n=4, **kw)
        assert o.rc == -5, kw
        assert o.counter.tolist() == [c.T] * 4 and all(bool((v == POISON).all()) for v in (o.actions, o.chunk, o.latent_out)), kw
    ok = Launch(dev, c, n=4)
    assert ok.rc == 0 and ok.counter.tolist() == [1] * 4 and torch.isfinite(ok.chunk).all()


def test_other_shapes_take_the_torch_path(dev, monkeypatch):
    """A width the kernel is not built for: the policy does not call the entry (which would refuse) but runs the torch path, on the device, on the same Philox stream."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_ACT_FUSED", raising=False)
    pol = P.ACTPolicy.random(4, 2, 3, device=dev, seed=2, enc_layers=1, dec_layers=1, hidden_dim=128, policy_seed=3)
    obs = torch.randn(3, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    assert not pol.fused_ok(obs)
    with pytest.warns(UserWarning, match="torch path"):
        y = pol.predict_batch(obs)
    assert y.shape == (3, 2) and torch.isfinite(y).all() and pol._packed.key is None and pol.counter.tolist() == [1, 1, 1]
    assert np.array_equal(pol.last_latent.cpu().numpy(), P.act_latent_uniforms(3, 0, 3, 0))
