"""d3il_bc_gmm (csrc/policy_bc_gmm.h) on the GPU through capi.launch against the f64 restatement of tests/bc_gmm_cases.py, the draws given (u_in, z_in) or made on
the device (Philox).  257 environments = 16 full 16-row tiles and a tail of one; launches of 1, 15, 16 and 17 rows must equal the first rows of the 257-row launch
bit for bit.  The yardstick of every accuracy assertion is the deviation of torch's own f32 evaluation (the policy's torch path on the device) from the f64
result on the same rows, per case, measured here and printed.  A banked u within BC_GMM_EDGE of an edge of the row's f64 normalised CDF is drawn again, so the
components are compared on EVERY row; only the device-drawn launch leaves rows out - at most DRAWN_CAP, a count the CPU suite pins for the same constants."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS = (1, 15, 16, 17)
STD_MODE = {"low_noise": 0, "exp": 1, "softplus": 2}
_DEV = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def on_device(c, dev):
    """The case's packed tables and constants on the device, and torch's f32 result there (computed once per case object)."""
    key = id(c)
    if key not in _DEV:
        pk = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in c.pol._pack().items()}
        consts = tuple(v.to(dev).contiguous() for v in (c.pol.lo, c.pol.hi, c.pol.out_scale, c.pol.out_shift))
        on = copy.copy(c.pol)
        on.model = copy.deepcopy(c.pol.model).to(dev)
        on.lo, on.hi, on.out_scale, on.out_shift = consts
        t32, k32, _ = on._predict_torch(c.state.to(dev), c.u.to(dev), c.z.to(dev))
        _DEV[key] = (c, pk, consts, on, t32.cpu(), k32.cpu())
    return _DEV[key][1:]


class Launch:
    """One call of the entry through capi.launch.  ``u`` / ``z``: "bank" = the case's banks, None = Philox, or a tensor.  Outputs are filled with 777 before the call;
    ``err`` is the D3ilError of a refused call."""

    def __init__(self, dev, c, n=None, first=0, state=None, u="bank", z="bank", seed=0, t=0, t_dev=None, env_offset=0, probs=True, **over):
        from d3il_amd import capi
        from tests.bc_gmm_cases import N
        n = N if n is None else n
        pk, (lo, hi, sc, sh) = on_device(c, dev)[:2]
        st = (c.state if state is None else state)[first:first + n].to(dev).contiguous()
        pick = lambda v, bank: None if v is None else (bank if isinstance(v, str) else v)[first:first + n].to(device=dev, dtype=torch.float32).contiguous()
        ut, zt = pick(u, c.u), pick(z, c.z)
        word = t_dev if t_dev is not None else torch.tensor([t - (1 << 32) if t >> 31 else t], dtype=torch.int32, device=dev)      # (the u32 word in an i32 tensor)
        A, G = over.get("A", c.A), over.get("G", c.G)
        mode = over.get("std_mode", STD_MODE[c.std])
        act = torch.full((n, max(c.A, A, 1)), 777.0, device=dev)
        comps = torch.full((n,), 777, dtype=torch.int32, device=dev)
        uo, zo = torch.full((n,), 777.0, device=dev), torch.full((n, max(c.A, A, 1)), 777.0, device=dev)
        pr = torch.full((n, max(c.G, G, 1)), 777.0, device=dev)
        self.err = None
        try:
            capi.launch("d3il_bc_gmm", dev, n_env=n, t_device=word, state=st, w_in=pk["w_in"], b_in=pk["b_in"], w_blocks=pk["w_blk"], b_blocks=pk["b_blk"], w_feat=pk["w_feat"],
                        b_feat=pk["b_feat"], w_logit=pk["w_logit"], b_logit=pk["b_logit"], w_mean=pk["w_mean"], b_mean=pk["b_mean"], w_std=None if mode == 0 else pk["w_std"],
                        b_std=None if mode == 0 else pk["b_std"], lo=lo, hi=hi, scale=sc, shift=sh, seed=seed, env_offset=env_offset, u_in=ut, z_in=zt, actions=act, comps=comps,
                        u_out=uo, z_out=zo, probs=pr if probs else None, obs_dim=over.get("obs", c.obs), G=G, A=A, hidden=over.get("hidden", c.hidden),
                        n_blocks=over.get("nblk", c.nblk), std_mode=mode, min_std=c.pol.min_std)
        except capi.D3ilError as e:
            self.err = str(e)
        torch.cuda.synchronize()
        self.raw = (act.cpu(), comps.cpu(), uo.cpu(), zo.cpu(), pr.cpu())
        self.actions, self.comps, self.u_out, self.z_out, self.probs = act[:, :c.A].cpu().contiguous(), comps.cpu(), uo.cpu(), zo[:, :c.A].cpu().contiguous(), pr[:, :c.G].cpu()

    def bits(self):
        return self.actions.numpy().view(np.uint32), self.comps.numpy(), self.u_out.numpy().view(np.uint32), self.z_out.numpy().view(np.uint32)

    def untouched(self):
        return all(bool((v == 777).all()) for v in self.raw)


def names():
    from tests.bc_gmm_cases import CASES
    return list(CASES)


@pytest.mark.parametrize("name", names())
def test_components_and_actions_against_f64(dev, name):
    from tests import bc_gmm_cases as B
    c = B.case(name)
    _, _, _, t32, k32 = on_device(c, dev)
    yard = float((t32.double() - c.want).abs().max())
    whole = Launch(dev, c)
    assert whole.err is None
    assert torch.equal(k32, c.comps)      # (torch's f32 layers agree on the bank too: the EDGE margin)
    assert torch.equal(whole.comps, c.comps)      # every row
    assert np.array_equal(whole.u_out.numpy().view(np.uint32), c.u.numpy().view(np.uint32)) and np.array_equal(whole.z_out.numpy().view(np.uint32), c.z.numpy().view(np.uint32))
    err = float((whole.actions.double() - c.want).abs().max())
    err_p = float((whole.probs.double() - c.p64).abs().max())
    sums = float((whole.probs.double().sum(dim=1) - 1).abs().max())
    # the clamp: a sample the f64 restatement puts clearly past a bound comes out as exactly that bound's action (f64 product and sum on the f32 operands, rounded once)
    lo, hi, sc, sh = (v.double() for v in (c.pol.lo, c.pol.hi, c.pol.out_scale, c.pol.out_shift))
    at_lo, at_hi = c.want == lo * sc + sh, c.want == hi * sc + sh
    y_lo, y_hi = (lo * sc + sh).float().expand(B.N, c.A), (hi * sc + sh).float().expand(B.N, c.A)
    print("%s: actions kernel %.3e, torch f32 %.3e -> %.2f yardsticks; probabilities %.2e, |sum p - 1| %.2e; %d / %d of %d samples on the lower / upper bound, %d distinct components, "
          "%d u redrawn" % (name, err, yard, err / yard, err_p, sums, int(at_lo.sum()), int(at_hi.sum()), c.want.numel(), len(set(c.comps.tolist())), c.redrawn))
    assert yard > 0 and err <= 4 * yard
    assert sums < 1e-5 and err_p < 1e-5      # G quotients each within 2^-24 relative of p / S, S a G-term f32 sum
    assert at_lo.any() and at_hi.any() and not (at_lo | at_hi).all()
    # no action lies beyond a bound's, the bound's action is attained exactly, and on the rows the restatement clamps (a sample within an f32 rounding of a bound aside)
    assert bool((whole.actions >= y_lo).all()) and bool((whole.actions <= y_hi).all())
    assert int(((whole.actions == y_lo) != at_lo).sum()) + int(((whole.actions == y_hi) != at_hi).sum()) <= 2
    assert c.G == 1 or len(set(c.comps.tolist())) > c.G // 2
    # every row count: the rows of a smaller launch are the rows of the whole one, bit for bit in every output
    for n in ROWS:
        part = Launch(dev, c, n=n)
        assert part.err is None
        for a, b in zip(part.bits(), whole.bits()):
            assert np.array_equal(a, b[:n]), n
    for a, b in zip(Launch(dev, c, probs=False).bits(), whole.bits()):      # without probs: the same other outputs
        assert np.array_equal(a, b)


def test_device_draws_are_the_host_generators(dev):
    """u_in / z_in NULL at a non-zero offset and step word and a 64-bit seed: u_out is bc_gmm_uniforms bit for bit, z_out is bc_gmm_normals to f32 Box-Muller accuracy
    (yardstick: torch's f32 Box-Muller on the same words against f64); components and actions are the f64 restatement's on those draws, the DRAWN_NEAR rows within
    EDGE of a CDF edge aside; rows 5 .. 8 equal a 4-row launch at env_offset + 5; the step word, the seed and the offset reach the counter."""
    from d3il_amd import policies as P
    from tests import bc_gmm_cases as B
    c, u, z64, _, near = B.drawn_reference()
    seed, t, off = B.DRAWN_SEED, B.DRAWN_T, B.DRAWN_OFFSET
    out = Launch(dev, c, u=None, z=None, seed=seed, t=t, env_offset=off)
    assert out.err is None
    assert np.array_equal(out.u_out.numpy(), u.numpy())      # bit for bit
    r = torch.as_tensor(P.bc_gmm_words(seed, off, B.N, t)[:, 1:3].astype(np.int64))
    u1, u2 = ((r[..., 0::2] >> 8) + 1).float() * 2.0 ** -24, (r[..., 1::2] >> 8).float() * 2.0 ** -24
    rad, ang = torch.sqrt(-2.0 * torch.log(u1)), 6.28318530717958647692 * u2
    z32 = torch.stack((rad * torch.cos(ang), rad * torch.sin(ang)), dim=-1).reshape(B.N, 8)[:, :c.A]
    yard_z = float((z32.double() - z64).abs().max())
    err_z = float((out.z_out.double() - z64).abs().max())
    assert yard_z > 0 and err_z <= 4 * yard_z
    # the restatement on the draws the kernel used (z_out: within the bar above of the host's)
    y64, k64, _ = c.reference(out.u_out, out.z_out)
    _, _, on, _, _ = on_device(c, dev)
    t32 = on._predict_torch(c.state.to(dev), out.u_out.to(dev), out.z_out.to(dev))[0].cpu()
    keep = ~near
    yard = float((t32.double() - y64)[keep].abs().max())
    err = float((out.actions.double() - y64)[keep].abs().max())
    print("device draws: z kernel %.3e torch f32 %.3e -> %.2f yardsticks; actions kernel %.3e torch f32 %.3e -> %.2f yardsticks; %d of %d rows within EDGE of a CDF edge"
          % (err_z, yard_z, err_z / yard_z, err, yard, err / yard, int(near.sum()), B.N))
    assert int(near.sum()) == B.DRAWN_NEAR <= B.DRAWN_CAP
    assert torch.equal(out.comps[keep], k64[keep]) and bool(((out.comps[near] - k64[near]).abs() <= 1).all())
    assert yard > 0 and err <= 4 * yard
    part = Launch(dev, c, n=4, first=5, u=None, z=None, seed=seed, t=t, env_offset=off + 5)
    for a, b in zip(part.bits(), out.bits()):
        assert np.array_equal(a, b[5:9])
    # the same launch with u_out / z_out handed back
    for a, b in zip(Launch(dev, c, u=out.u_out, z=out.z_out).bits(), out.bits()):
        assert np.array_equal(a, b)
    # the device step word: advanced -> the draws of t + 1; seed and offset reach the counter
    word = torch.tensor([7], dtype=torch.int32, device=dev)
    a = Launch(dev, c, n=17, u=None, z=None, seed=seed, t_dev=word)
    word.add_(1)
    b = Launch(dev, c, n=17, u=None, z=None, seed=seed, t_dev=word)
    assert np.array_equal(a.u_out.numpy(), P.bc_gmm_uniforms(seed, 0, 17, 7)) and np.array_equal(b.u_out.numpy(), P.bc_gmm_uniforms(seed, 0, 17, 8))
    assert not torch.equal(a.z_out, b.z_out) and not torch.equal(Launch(dev, c, n=17, u=None, z=None, seed=seed + 1, t=7).u_out, a.u_out)
    assert not torch.equal(Launch(dev, c, n=17, u=None, z=None, seed=seed, t=7, env_offset=1 << 32).u_out, a.u_out)


def test_std_mlp_is_never_read_in_low_noise_mode(dev):
    """NULL for w_std / b_std (what Launch passes in that mode) and std = 1e-4 exactly: the sample is mean + 1e-4 z."""
    from tests import bc_gmm_cases as B
    c = B.case("h128b3_o4a2g8_low")
    a = Launch(dev, c, n=33)
    zero = Launch(dev, c, n=33, z=torch.zeros(B.N, c.A))
    assert a.err is None and zero.err is None and torch.equal(a.comps, zero.comps)
    y0 = c.reference(c.u[:33], torch.zeros(33, c.A), c.state[:33])[0]
    on = on_device(c, dev)[2]
    t32 = on._predict_torch(c.state[:33].to(dev), c.u[:33].to(dev), torch.zeros(33, c.A, device=dev))[0].cpu()
    yard = float((t32.double() - y0).abs().max())
    assert yard > 0 and float((zero.actions.double() - y0).abs().max()) <= 4 * yard      # the means alone, on the same 33 rows
    assert not torch.equal(a.actions, zero.actions)


@pytest.mark.parametrize("name", ["h128b3_o4a2g8_low", "h256b0_o28a8g64_exp"])
def test_nonfinite_values_mark_their_environment_only(dev, name):
    from tests import bc_gmm_cases as B
    c = B.case(name)
    clean = Launch(dev, c)
    assert torch.isfinite(clean.actions).all() and (clean.comps >= 0).all()
    state, z = c.state.clone(), c.z.clone()
    state[3, c.obs - 1], state[9, 0], state[256, 0] = float("nan"), float("inf"), float("-inf")      # (256: the lone row of the last workgroup)
    z[20, c.A - 1], z[21, 0] = float("nan"), float("inf")      # a used draw
    bad = Launch(dev, c, state=state, z=z)
    hit = [3, 9, 20, 21, 256]
    good = [r for r in range(B.N) if r not in hit]
    assert np.array_equal(bad.actions[hit].numpy().view(np.uint32), np.full((5, c.A), 0x7FC00000, dtype=np.uint32))
    assert bad.comps[hit].tolist() == [-1] * 5
    for a, b in zip(bad.bits()[:3], clean.bits()[:3]):
        assert np.array_equal(a[good], b[good])
    assert np.array_equal(bad.bits()[2], clean.bits()[2])      # u_out is the uniform, hit or not


def test_an_overflowing_input_layer_marks_its_environment(dev):
    """A finite state whose hidden row leaves the f32 range (the input layer's weights times 1e4, one row's state at 3e37): component -1 and NaN for that row, every
    other row as without it."""
    from tests import bc_gmm_cases as B
    def tweak(model):
        model.mlp.layers[0].weight.mul_(1e4)
    c = B.Case("h128b3_o4a2g8_low", tweak=tweak)
    clean = Launch(dev, c, n=33)
    state = c.state.clone()
    state[18] = 3e37
    out = Launch(dev, c, n=33, state=state)
    good = [r for r in range(33) if r != 18]
    assert np.array_equal(out.bits()[0][18], np.full(c.A, 0x7FC00000, dtype=np.uint32)) and int(out.comps[18]) == -1
    assert (clean.comps >= 0).all()
    for a, b in zip(out.bits(), clean.bits()):
        assert np.array_equal(a[good], b[good])


def test_an_overflowing_exp_std_marks_its_environment(dev):
    """std = exp(100) = Inf in one component's std row: the clamp would turn mean + Inf z into a bound; the rows that draw this component are marked instead, every
    other row is bit-equal to the launch without the overflow."""
    from tests import bc_gmm_cases as B
    base = B.case("h256b3_o20a3g17_exp")
    k = int(base.comps[7])
    def tweak(model):
        model.std_mlp.bias[k * base.A + 1] = 100.0
    c = B.Case("h256b3_o20a3g17_exp", tweak=tweak)
    assert torch.equal(c.u, base.u) and torch.equal(c.z, base.z)      # (the logits do not depend on the std head: the same banks)
    clean, out = Launch(dev, base, n=65), Launch(dev, c, n=65, u=base.u)
    hit = [r for r in range(65) if int(base.comps[r]) == k]
    good = [r for r in range(65) if r not in hit]
    assert 7 in hit and good
    assert np.array_equal(out.bits()[0][hit], np.full((len(hit), c.A), 0x7FC00000, dtype=np.uint32)) and out.comps[hit].tolist() == [-1] * len(hit)
    for a, b in zip(out.bits(), clean.bits()):
        assert np.array_equal(a[good], b[good])


def test_unsupported_shapes_are_refused_before_any_launch(dev):
    from tests import bc_gmm_cases as B
    c = B.case("h128b3_o4a2g8_low")
    for kw in (dict(hidden=192), dict(G=0), dict(G=65), dict(A=0), dict(A=9), dict(obs=29), dict(nblk=-1), dict(std_mode=3)):
        o = Launch(dev, c, n=4, **kw)
        assert o.err is not None and "error -5" in o.err and "d3il_bc_gmm" in o.err, kw
        assert o.untouched(), kw
    ok = Launch(dev, c, n=4)
    assert ok.err is None and torch.isfinite(ok.actions).all() and not ok.untouched() and (ok.comps != 777).all()


def test_an_unsupported_network_takes_torchs_layers(dev, monkeypatch):
    """A hidden width the kernel is not built for: the policy does not call the entry (which would refuse) but runs torch's layers, on the device, and says so once."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_BC_GMM_FUSED", raising=False)
    pol = P.BCGMMPolicy.random(4, 2, device=dev, seed=2, hidden_dim=64, n_blocks=1, policy_seed=3)
    obs = torch.randn(3, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    assert not pol.fused_ok(obs)
    with pytest.warns(UserWarning, match="torch's layers"):
        y = pol.predict_batch(obs)
    assert y.shape == (3, 2) and torch.isfinite(y).all() and pol._packed.key is None
    assert np.array_equal(pol.last_u.cpu().numpy(), P.bc_gmm_uniforms(3, 0, 3, 0))
