"""policies.DDPMACTPolicy on the CPU against the reference's own enc-dec DiffusionAgent + Diffusion + DiffusionEncDec: tests/golden/ref_ddpm_act_agent.npz holds a
scaler and, for two cases, observations, a noise bank and the reference rolled out batch-1 per environment TWICE - in f32 as shipped and in f64
(tests/golden/gen_ddpm_act_goldens.py, run where the reference is).  The weights are not stored: policies.ddpm_act_synthetic_state rebuilds them and the fixture's
checksum proves it.  D = max |f32 - f64| of the reference's own actions is the yardstick of a case; the replay must stay within 4 D of the f64 table with identical
counters, window lengths and chunk hand-over, including the reset that lands mid-chunk.  The device replay of the same fixture is tests/test_gpu_policies_ddpm_act.py."""
import math
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch.nn import functional as F  # noqa: E402
from d3il_amd import policies as P  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ddpm_act_agent.npz"))
CFG_KEYS = ("OBS", "C", "HEADS", "ENC", "DEC", "S", "Ta", "A", "T", "WINDOW", "SEED", "n_env", "n_steps", "reset_env", "reset_step")
_SD = {}


def cfg(case):
    return types.SimpleNamespace(**{k: int(v) for k, v in zip(CFG_KEYS, G["da_%s_cfg" % case])}, D=float(G["da_%s_D" % case]), p="da_%s_" % case)


def golden_sd(case):
    """The generator's weights of a case, rebuilt (shared by the tests of this module and of the GPU modules; never modified)."""
    if case not in _SD:
        c = cfg(case)
        _SD[case] = P.ddpm_act_synthetic_state(P.ddpm_act_reference_shapes(c.OBS, c.A, c.S, c.Ta, c.C, c.ENC, c.DEC), c.SEED)
    return _SD[case]


def golden_net(case):
    c = cfg(case)
    net = P.EncDecDenoiser(c.OBS, c.A, c.C, c.HEADS, c.ENC, c.DEC, c.S, c.Ta, c.WINDOW + 1)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in golden_sd(case).items()})
    return net


def golden_policy(case, dev, seed=0, **kw):
    c = cfg(case)
    sc = P.Scaler(G["da_x_mean"], G["da_x_std"], G["da_y_mean"], G["da_y_std"], G["da_y_bounds"], device=dev)
    pol = P.DDPMACTPolicy(golden_net(case).to(dev), sc, c.T, seed=seed, **kw)
    for p in pol.model.parameters():
        p.requires_grad_(False)
    return pol


class Bank:
    """noise_in that replays the golden bank of step ``t``."""

    def __init__(self, case):
        self.t = 0
        self.noise_in = lambda n: G["da_%s_noise" % case][:n, self.t]


def replay(case, dev):
    """The golden rollout of a case as ONE batch on ``dev``: (worst action deviation from the f64 table, worst chunk deviation, counters / lengths equal, clamp
    entries exact, their number, policy).  Every row of every step is compared; the chunk table is compared after every step (hand-over included)."""
    c, b = cfg(case), Bank(case)
    pol = golden_policy(case, dev, noise_in=b.noise_in)
    pol.record = True
    obs = G[c.p + "obs"]
    lo, hi = G["da_y_bounds"]
    scale64, shift64 = G["da_y_std"] + 1e-12, G["da_y_mean"]
    edge = (pol.lo.cpu() * pol.out_scale.cpu() + pol.out_shift.cpu(), pol.hi.cpu() * pol.out_scale.cpu() + pol.out_shift.cpu())      # a bound through the two f32 operations
    wa = wc = 0.0
    same = exact = True
    n_edge = 0
    for t in range(c.n_steps):
        b.t = t
        if t == c.reset_step:
            mask = torch.zeros(c.n_env, dtype=torch.bool)
            mask[c.reset_env] = True
            pol.begin_episodes(mask.to(dev))
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        wa = max(wa, float(np.abs(a - G[c.p + "ref64"][:, t]).max()))
        same = same and np.array_equal(pol.counter.cpu().numpy().astype(np.int64), G[c.p + "counter"][:, t]) and np.array_equal(pol.hist.len.cpu().numpy(), G[c.p + "len"][:, t])
        same = same and not bool(pol.last_bad.any())
        ch = pol.last_chunk.cpu()
        want = G[c.p + "chunks64"][:, t]
        wc = max(wc, float(np.abs(ch.numpy().astype(np.float64) - want).max()))
        scaled = (want - shift64) / scale64
        at_lo, at_hi = torch.as_tensor(scaled <= lo + 1e-9), torch.as_tensor(scaled >= hi - 1e-9)
        n_edge += int(at_lo.sum() + at_hi.sum())
        exact = exact and torch.equal(ch[at_lo], edge[0].expand_as(ch)[at_lo]) and torch.equal(ch[at_hi], edge[1].expand_as(ch)[at_hi])
    return wa, wc, same, exact, n_edge, pol


@pytest.mark.parametrize("case", ["a", "b"])
def test_rebuilt_weights_are_the_generators(case):
    c, sd = cfg(case), golden_sd(case)
    keys = sorted(sd)
    sums = np.array([float(np.asarray(sd[k], dtype=np.float64).sum()) for k in keys])
    assert len(keys) == len(G[c.p + "w_sums"]) and np.array_equal(sums, G[c.p + "w_sums"])
    for (i, j), want in zip(G["da_w_probe_at"], G[c.p + "w_probes"]):
        assert float(sd[keys[int(i)]].reshape(-1)[int(j)]) == float(want)
    net = golden_net(case)
    assert [k for k, _ in net.named_parameters()] == list(P.ddpm_act_reference_shapes(c.OBS, c.A, c.S, c.Ta, c.C, c.ENC, c.DEC)) and set(net.state_dict()) == set(keys)
    assert all(sd[k].dtype == np.float32 for k in keys)
    assert (c.C, c.HEADS, c.ENC, c.DEC, c.S, c.WINDOW, c.OBS, c.A) == (64, 4, 2, 4, 5, 8, 10, 2)      # the shipped network at obs 10, A 2


@pytest.mark.parametrize("case", ["a", "b"])
def test_policy_rows_equal_reference_predict(case):
    """Whole chains, both cases, every row: within 4 D of the reference's f64 run."""
    c = cfg(case)
    assert float(np.abs(G[c.p + "ref32"] - G[c.p + "ref64"]).max()) == c.D and G[c.p + "ref64"].shape == (c.n_env, c.n_steps, c.A)
    if case == "a":
        assert (c.Ta, c.T, c.n_env, c.n_steps, c.reset_env, c.reset_step) == (4, 16, 4, 10, 2, 6)
        assert G[c.p + "computed"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0] and G[c.p + "computed"][2].tolist() == [1, 0, 0, 0, 1, 0, 1, 0, 0, 0]      # the reset lands mid-chunk
        assert sorted(set(G[c.p + "len"][G[c.p + "computed"] == 1].tolist())) == [1, 5]
    else:
        assert (c.Ta, c.T, c.n_env, c.n_steps) == (2, 4, 3, 6) and sorted(set(G[c.p + "len"][G[c.p + "computed"] == 1].tolist())) == [1, 3, 5]
    wa, wc, same, exact, n_edge, pol = replay(case, "cpu")
    print("golden replay %s (cpu): actions %.3e = %.2f D, chunks %.3e = %.2f D (D %.3e); %d chunk entries on a clamp bound" % (case, wa, wa / c.D, wc, wc / c.D, c.D, n_edge))
    assert same and exact and n_edge > 0
    assert wa <= 4 * c.D and wc <= 4 * c.D
    assert int(pol._t) == c.n_steps


def formula(sd, x, i, states, heads=4):
    """DiffusionEncDec.forward without goals written out on the state dict alone, shaped as the reference writes it: returns (eps, encoder output)."""
    Cw = sd["tok_emb.weight"].shape[0]
    hd = Cw // heads
    lin = lambda v, p: v @ sd[p + ".weight"].T + sd[p + ".bias"]
    ln = lambda v, p: F.layer_norm(v, (Cw,), sd[p + ".weight"], None, 1e-5)
    sp = lambda v: v.view(v.shape[0], -1, heads, hd).transpose(1, 2)
    tri = torch.tril(torch.ones(9, 9)).view(1, 1, 9, 9)

    def attend(q, k, v, mask):
        att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hd))
        if mask is not None:
            att = att.masked_fill(mask == 0, float("-inf"))
        return torch.softmax(att, dim=-1) @ v

    def block(v, p, cond):
        h = ln(v, p + "ln1")
        n_ = h.shape[1]
        y = attend(sp(lin(h, p + "attn.query")), sp(lin(h, p + "attn.key")), sp(lin(h, p + "attn.value")), tri[:, :, :n_, :n_])
        if cond is not None:
            y = y + attend(sp(lin(h, p + "attn.cross_query")), sp(lin(cond, p + "attn.cross_key")), sp(lin(cond, p + "attn.cross_value")), None)
        v = v + lin(y.transpose(1, 2).reshape(v.shape), p + "attn.proj")
        return v + lin(F.gelu(lin(ln(v, p + "ln2"), p + "mlp.0")), p + "mlp.2")

    def stack(v, name, cond):
        l = 0
        while "%s.blocks.%d.ln1.weight" % (name, l) in sd:
            v = block(v, "%s.blocks.%d." % (name, l), cond)
            l += 1
        return ln(v, name + ".ln")

    b, L, _ = states.shape
    Ta = x.shape[1]
    half = Cw // 2
    freq = torch.exp(torch.arange(half, dtype=x.dtype) * -(math.log(10000) / (half - 1)))
    e = torch.full((b, 1), float(i), dtype=x.dtype) * freq
    te = lin(F.mish(lin(torch.cat((e.sin(), e.cos()), dim=-1), "time_emb.1")), "time_emb.3").unsqueeze(1)
    pos = sd["pos_emb"][:, :L + Ta - 1]
    enc = stack(torch.cat([te, lin(states, "tok_emb") + pos[:, :L]], dim=1), "encoder", None)
    return lin(stack(lin(x, "action_emb") + pos[:, L - 1:], "decoder", enc), "action_pred"), enc


@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("Ta", [1, 4])
def test_module_equals_the_reference_shaped_formula_in_f64(L, Ta):
    pol = P.DDPMACTPolicy.random(7, 3, device="cpu", seed=5, action_seq_len=Ta, n_timesteps=6)
    net = pol.model.double()
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    assert tuple(sd["pos_emb"].shape) == (1, 5 - 1 + Ta, 64)
    g = torch.Generator().manual_seed(1)
    x, states = torch.randn(4, Ta, 3, generator=g, dtype=torch.float64), torch.randn(4, L, 7, generator=g, dtype=torch.float64)
    for i in (0, 5):
        want, enc_want = formula(sd, x, i, states)
        time = torch.full((4,), i, dtype=torch.long)
        have, enc = net(x, time, states), net.encode(time, states)
        assert have.shape == (4, Ta, 3) and float((have - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert enc.shape == (4, 1 + L, 64) and float((enc - enc_want).abs().max()) <= 1e-12 * float(enc_want.abs().max())
        # the encoder output does not change with the iterate; the noise estimate does
        other, enc_other = formula(sd, x + 0.5, i, states)
        assert torch.equal(enc_other, enc_want) and float((other - want).abs().max()) > 1e-6
        assert torch.equal(net.decode(x, enc), have)
    # the action tokens take pos rows L - 1 .. L - 2 + Ta: moving any other row of the table changes nothing unless a state token reads it
    moved = {k: v.clone() for k, v in sd.items()}
    ramp = torch.linspace(-1.0, 1.0, 64, dtype=torch.float64)      # (a constant over the features would vanish in the next LayerNorm)
    moved["pos_emb"][0, L - 1 + Ta - 1] += ramp      # the last action token's row (a state row too only if Ta = 1)
    assert float((formula(moved, x, 2, states)[0] - formula(sd, x, 2, states)[0]).abs().max()) > 1e-6
    if L - 1 + Ta < sd["pos_emb"].shape[1]:
        beyond = {k: v.clone() for k, v in sd.items()}
        beyond["pos_emb"][0, L - 1 + Ta:] += ramp      # rows past the last action token are not read at this window length
        assert torch.equal(formula(beyond, x, 2, states)[0], formula(sd, x, 2, states)[0])
        net2 = P.EncDecDenoiser(7, 3, 64, 4, 2, 4, 5, Ta, 9).double()
        net2.load_state_dict(beyond)
        assert torch.equal(net2(x, torch.full((4,), 2), states), net(x, torch.full((4,), 2), states))


def test_chain_is_the_reference_sampler_written_out_in_f64():
    """_chain_torch against Diffusion.sample restated on the schedule tables in f64: x0 clipped, posterior mean, noise except at step 0, final clamp, two-step scaling."""
    pol = P.DDPMACTPolicy.random(6, 2, device="cpu", seed=4, n_timesteps=5, action_seq_len=3, bound=2.0)
    pol.model.double()
    g = torch.Generator().manual_seed(3)
    st, noise = torch.randn(3, 2, 6, generator=g, dtype=torch.float64), torch.randn(3, 6, 3, 2, generator=g, dtype=torch.float64)
    y, bad, x_last = pol._chain_torch(st, noise)
    s = P.ddpm_schedule(P.cosine_beta_schedule(5).double())
    x = noise[:, 5]
    for i in reversed(range(5)):
        eps = pol.model(x, torch.full((3,), i), st)
        x0 = (s["sqrt_recip_ac"][i] * x - s["sqrt_recipm1_ac"][i] * eps).clamp(-2.0, 2.0)
        x = s["coef1"][i] * x0 + s["coef2"][i] * x + (0.0 if i == 0 else 1.0) * (0.5 * s["post_logvar"][i]).exp() * noise[:, i]
    assert not bool(bad.any()) and float((x_last - x).abs().max()) <= 1e-13
    assert float((y - (x.clamp(-2.0, 2.0) * pol.out_scale.double() + pol.out_shift.double())).abs().max()) <= 1e-18
    # the hooks: steps 3 .. 2 from the iterate that entered step 3
    xs = [noise[:, 5]]
    for i in (4, 3, 2):
        xs.append(pol._chain_torch(st, noise, x=xs[-1], k_start=i, k_stop=i)[2])
    assert float((pol._chain_torch(st, noise, x=xs[1], k_start=3, k_stop=2)[2] - xs[3]).abs().max()) == 0.0


ENC_M, DEC_M = ("query", "key", "value", "proj"), ("query", "key", "value", "cross_query", "cross_key", "cross_value", "proj")


@pytest.mark.parametrize("obs,A_,S_,Ta,enc,dec,T_", [(4, 2, 1, 1, 1, 1, 2), (10, 2, 5, 4, 2, 4, 16), (32, 8, 5, 4, 2, 4, 4)])
def test_packer_index_by_index(obs, A_, S_, Ta, enc, dec, T_):
    """[To][t][lane (g, i)][r] = W[16 To + i][16 t + 4 g + r] for every matrix, the layer arrays in the order csrc/policy_act.h reads them, the table of
    csrc/policy_ddpm_act.h: position rows, final LayerNorms, biases, the time tokens of the module's own time_emb, the five schedule columns."""
    pol = P.DDPMACTPolicy.random(obs, A_, device="cpu", seed=3, obs_seq_len=S_, action_seq_len=Ta, enc_layers=enc, dec_layers=dec, n_timesteps=T_)
    net, pk = pol.model, pol._pack()
    assert pk["w_in"].shape == (3072,) and pk["tab"].shape == (784 + 69 * T_,) and pk["enc_w"].shape == (enc, 49152) and pk["enc_v"].shape == (enc, 704)
    assert pk["dec_w"].shape == (dec, 61440) and pk["dec_v"].shape == (dec, 896) and pk["head_w"].shape == (1024,) and all(v.dtype == torch.float32 for v in pk.values())
    rng = np.random.default_rng(0)
    at = lambda flat, off, Nt, To, t, g, i, r: float(flat[off + (((To * Nt + t) * 64) + 16 * g + i) * 4 + r])
    for _ in range(150):
        To, t, g, i, r = (int(rng.integers(0, m)) for m in (4, 4, 4, 16, 4))
        row, col = 16 * To + i, 16 * t + 4 * g + r
        if t < 2:
            assert at(pk["w_in"], 0, 2, To, t, g, i, r) == (float(net.tok_emb.weight[row, col]) if col < obs else 0.0)
        if t == 0:
            assert at(pk["w_in"], 2048, 1, To, 0, g, i, r) == (float(net.action_emb.weight[row, col]) if col < A_ else 0.0)
        if To == 0:
            assert at(pk["head_w"], 0, 4, 0, t, g, i, r) == (float(net.action_pred.weight[i, col]) if i < A_ else 0.0)
        for stack, names, key in ((net.encoder, ENC_M, "enc"), (net.decoder, DEC_M, "dec")):
            for l, b in enumerate(stack.blocks):
                for m, name in enumerate(names):
                    assert at(pk[key + "_w"][l], 4096 * m, 4, To, t, g, i, r) == float(getattr(b.attn, name).weight[row, col])
                    assert float(pk[key + "_v"][l][128 + 64 * m + row]) == float(getattr(b.attn, name).bias[row])
                nm = len(names)
                To1, t2 = int(rng.integers(0, 16)), int(rng.integers(0, 16))
                assert at(pk[key + "_w"][l], 4096 * nm, 4, To1, t, g, i, r) == float(b.mlp[0].weight[16 * To1 + i, col])
                assert at(pk[key + "_w"][l], 4096 * nm + 16384, 16, To, t2, g, i, r) == float(b.mlp[2].weight[row, 16 * t2 + 4 * g + r])
                v = pk[key + "_v"][l]
                assert float(v[row]) == float(b.ln1.weight[row]) and float(v[64 + row]) == float(b.ln2.weight[row])
                assert float(v[128 + 64 * nm + 16 * To1 + i]) == float(b.mlp[0].bias[16 * To1 + i]) and float(v[128 + 64 * nm + 256 + row]) == float(b.mlp[2].bias[row])
    tab, rows = pk["tab"], S_ - 1 + Ta
    assert torch.equal(tab[:64 * rows].reshape(rows, 64), net.pos_emb[0]) and float(tab[64 * rows:512].abs().sum()) == 0.0
    assert torch.equal(tab[512:576], net.encoder.ln.weight) and torch.equal(tab[576:640], net.decoder.ln.weight)
    assert torch.equal(tab[640:704], net.tok_emb.bias) and torch.equal(tab[704:768], net.action_emb.bias)
    assert torch.equal(tab[768:768 + A_], net.action_pred.bias) and float(tab[768 + A_:784].abs().sum()) == 0.0
    # the time tokens: the module's own time_emb (the nn.Sequential with the sinusoid in front) on the integer steps, in f32
    assert torch.equal(tab[784:784 + 64 * T_].reshape(T_, 64), net.time_emb(torch.arange(T_)))
    assert torch.equal(net.time_tokens(torch.arange(T_)), net.time_emb(torch.arange(T_)))
    sch = P.ddpm_schedule(P.cosine_beta_schedule(T_))
    sig = (0.5 * sch["post_logvar"]).exp()
    sig[0] = 0.0
    want = torch.stack((sch["sqrt_recip_ac"], sch["sqrt_recipm1_ac"], sch["coef1"], sch["coef2"], sig), dim=1)
    assert torch.equal(tab[784 + 64 * T_:].reshape(T_, 5), want) and torch.equal(pol._sched, want)


def test_host_generator():
    """The words are Philox4x32-10 of the stated counters; every counter field changes them; no tag collision; moments over 2^20 normals within 5 sigma."""
    seed, off, t = 0x1234567890ABCDEF, (1 << 32) - 3, 7
    w = P.ddpm_act_words(seed, off, 3, t, 9, 4)
    assert w.shape == (3, 4, 2, 4) and w.dtype == np.uint32
    for n in range(3):
        ge = off + n
        for j in range(4):
            for q in range(2):
                want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x44410000 | 9 << 8 | j << 1 | q)
                assert [int(x) for x in want] == w[n, j, q].tolist()
    z = P.ddpm_act_normals(seed, off, 3, t, 9, 4, 8)
    assert z.dtype == np.float64 and z.shape == (3, 4, 8)
    u1, u2 = ((int(w[2, 3, 1, 2]) >> 8) + 1) * 2.0 ** -24, (int(w[2, 3, 1, 3]) >> 8) * 2.0 ** -24
    assert abs(z[2, 3, 6] - math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2)) <= 1e-14 and abs(z[2, 3, 7] - math.sqrt(-2 * math.log(u1)) * math.sin(2 * math.pi * u2)) <= 1e-14
    assert np.array_equal(P.ddpm_act_normals(seed, off, 3, t, 9, 4, 2), z[:, :, :2]) and np.array_equal(P.ddpm_act_normals(seed, off, 3, t, 9, 2, 8), z[:, :2])
    base = P.ddpm_act_words(seed, 0, 4, t, 9, 4)
    for other in (P.ddpm_act_words(seed + 1, 0, 4, t, 9, 4), P.ddpm_act_words(seed, 4, 4, t, 9, 4), P.ddpm_act_words(seed, 0, 4, t + 1, 9, 4), P.ddpm_act_words(seed ^ (1 << 40), 0, 4, t, 9, 4),
                  P.ddpm_act_words(seed, 1 << 32, 4, t, 9, 4), P.ddpm_act_words(seed, 0, 4, t, 10, 4)):
        assert not np.isin(other, base).any()
    assert np.array_equal(P.ddpm_act_words(seed, 1, 3, t, 9, 4), base[1:]) and len({tuple(x) for x in base.reshape(-1, 4)}) == 4 * 4 * 2
    with pytest.raises(AssertionError):
        P.ddpm_act_words(seed, 0, 1, t, 0, 4)      # chain index 0 is never drawn
    # the tag: no word of this kernel equals a word of the five others, and none is 0
    tags = {P.DDPM_ACT_TAG | k << 8 | j << 1 | q for k in range(1, 256) for j in range(4) for q in range(2)}
    gpt = {P.DDPM_GPT_TAG | k << 8 | j << 1 | q for k in range(1, 256) for j in range(16) for q in range(2)}
    ibc = {P.IBC_TAG | kind << 14 | kk << 8 | s << 2 | q for kind in range(3) for kk in range(64) for s in range(64) for q in range(2)}
    small = {P.ACT_TAG | q for q in range(8)} | {P.CVAE_TAG | q for q in range(8)} | {P.BET_TAG}
    assert P.DDPM_ACT_TAG == 0x44410000 and 0 not in tags and not tags & gpt and not tags & ibc and not tags & small
    assert len({P.DDPM_ACT_TAG, P.DDPM_GPT_TAG, P.IBC_TAG, P.ACT_TAG, P.CVAE_TAG, P.BET_TAG}) == 6
    from d3il_amd import capi
    assert capi.DDPM_ACT_TAG == P.DDPM_ACT_TAG
    zz = np.concatenate([P.ddpm_act_normals(3, 0, 1 << 13, tt, k, 4, 8).reshape(-1) for tt in range(2) for k in (1, 16)])
    m = zz.size
    print("moments over %d normals: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e)" % (m, zz.mean(), 5 / np.sqrt(m), zz.var() - 1, 5 * np.sqrt(2 / m)))
    assert m >= 1 << 20 and np.isfinite(zz).all()
    assert abs(zz.mean()) < 5 / np.sqrt(m) and abs(zz.var() - 1) < 5 * np.sqrt(2 / m) and abs((zz ** 3).mean()) < 5 * np.sqrt(15 / m)


def fake_agent(case="a", ema=False, **over):
    """A duck-typed enc-dec DiffusionAgent around the golden network of a case."""
    c = cfg(case)
    net = golden_net(case)
    sc = types.SimpleNamespace(x_mean=G["da_x_mean"], x_std=G["da_x_std"], y_mean=G["da_y_mean"], y_std=G["da_y_std"], y_bounds=G["da_y_bounds"])
    diff = types.SimpleNamespace(model=net, n_timesteps=c.T, betas=P.cosine_beta_schedule(c.T), predict_epsilon=True, clip_denoised=True, diffusion_x=False)
    ag = types.SimpleNamespace(model=diff, scaler=sc, obs_seq_len=c.S, action_seq_size=c.Ta, action_counter=c.Ta, window_size=c.WINDOW, diffusion_kde=False, use_ema=ema,
                               goal_condition=False, predict=lambda s: None, reset=lambda: None)
    if ema:      # the live weights are something else; the shadow list holds the golden ones
        ag.ema_helper = types.SimpleNamespace(shadow_params=[p.detach().clone() for p in net.parameters()])
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(0.5)
    for k, v in over.items():
        setattr(ag, k, v)
    return ag


def test_from_reference_and_adapter_selection():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = fake_agent()
    assert P.DDPMACTPolicy.matches(agent) and P.DDPMACTPolicy.matches(fake_agent("b"))
    assert not any(pol.matches(agent) for pol in (P.BeTPolicy, P.DDPMGPTPolicy, P.IBCPolicy, P.ACTPolicy, P.CVAEPolicy))
    def with_diff(**kw):
        ag = fake_agent()
        for k, v in kw.items():
            setattr(ag.model, k, v)
        return ag
    goal = fake_agent()
    goal.model.model.goal_conditioned = True
    gpt = fake_agent()
    gpt.model.model = P.DiffusionGPTDenoiser(10, 2, 64, 2, 4, 5)
    mlp = fake_agent()
    mlp.model.model = P.DiffusionMLP(2, 10, 8, 64, 2)
    short = fake_agent()
    for b in list(short.model.model.encoder.blocks) + list(short.model.model.decoder.blocks):
        b.attn.mask = torch.tril(torch.ones(4, 4)).view(1, 1, 4, 4)      # masks narrower than 1 + obs_seq_len tokens
    others = {"goal conditioned": goal, "diffusion_x": with_diff(diffusion_x=True), "diffusion_kde": fake_agent(diffusion_kde=True), "x0 prediction": with_diff(predict_epsilon=False),
              "clip off": with_diff(clip_denoised=False), "other betas": with_diff(betas=torch.linspace(1e-4, 2e-2, 16)), "GPT denoiser": gpt, "MLP denoiser": mlp,
              "chunk != model": fake_agent(action_seq_size=3), "window > model": fake_agent(obs_seq_len=6), "narrow masks": short}
    for name, other in others.items():
        assert not P.DDPMACTPolicy.matches(other), name
        if name not in ("GPT denoiser",):
            assert isinstance(as_batched(other, 2), RowwiseAgent), name
    assert P.DDPMGPTPolicy.matches(gpt) and not P.DDPMGPTPolicy.matches(agent)      # each sampler keeps to its own denoiser
    pol = as_batched(agent, 4)
    c = cfg("a")
    assert isinstance(pol, P.DDPMACTPolicy) and (pol.T, pol.Ta, pol.S, pol.A, pol.obs_dim) == (c.T, c.Ta, c.S, c.A, c.OBS) and pol.counter.tolist() == [c.Ta] * 4
    assert pol.hist.len.tolist() == [0] * 4 and pol.model.block_size == c.WINDOW + 1
    # the converted agent replays the golden rows of step 0 - from the live weights, and from the EMA shadow list when use_ema is set
    for ema in (False, True):
        b = Bank("a")
        ag = fake_agent(ema=ema)
        pol = P.DDPMACTPolicy.from_reference(ag, noise_in=b.noise_in)
        a = pol.predict_batch(torch.as_tensor(G["da_a_obs"][:, 0])).numpy().astype(np.float64)
        assert float(np.abs(a - G["da_a_ref64"][:, 0]).max()) <= 4 * c.D, ema
        assert ag.model.model is not pol.model      # a copy: the agent's own module is left alone
    with pytest.raises((AssertionError, RuntimeError)):
        pol.predict_batch(torch.zeros(2, c.OBS + 1))


def test_fork_ranges_and_episode_masks():
    c = cfg("b")
    obs = torch.as_tensor(G["da_b_obs"])
    whole, part = golden_policy("b", "cpu", seed=5), golden_policy("b", "cpu", seed=5)
    whole.record = part.record = True
    part.set_rollout_range(1, 2)
    assert part.counter.tolist() == [c.Ta] * 2 and part.env_offset == 1 and part.hist.len.tolist() == [0, 0]
    for s in range(4):
        if s == 3:
            whole.begin_episodes(torch.tensor([False, False, True]))
            part.begin_episodes(torch.tensor([False, True]))
            assert whole.counter.tolist() == [1, 1, c.Ta] and whole.hist.len.tolist() == [3, 3, 0]
        a, b = whole.predict_batch(obs[:, s]), part.predict_batch(obs[1:3, s])
        assert torch.equal(whole.last_noise[1:3], part.last_noise) and torch.equal(whole.counter[1:3], part.counter) and torch.equal(whole.hist.len[1:3], part.hist.len)
        assert float((a[1:3] - b).abs().max()) <= 4 * c.D      # (torch's CPU GEMM may round a 3-row and a 2-row batch differently; the draws are identical)
        if s == 0:
            for k in range(1, c.T + 1):
                assert np.array_equal(whole.last_noise[:, k].numpy(), P.ddpm_act_normals(5, 0, 3, 0, k, c.Ta, c.A).astype(np.float32))
            assert float(whole.last_noise[:, 0].abs().sum()) == 0.0
        if s == 1:      # nobody is due: nothing is drawn
            assert float(whole.last_noise.abs().sum()) == 0.0
        if s == 3:      # only lane 2 draws, at step word 3, with a window of one entry
            assert np.array_equal(whole.last_noise[2, c.T].numpy(), P.ddpm_act_normals(5, 0, 3, 3, c.T, c.Ta, c.A).astype(np.float32)[2]) and float(whole.last_noise[:2].abs().sum()) == 0.0
    assert whole.counter.tolist() == [2, 2, 1] and whole.hist.len.tolist() == [4, 4, 1]
    # fork: network shared; per-lane state, window, step word and packed buffers its own
    twin = whole.fork()
    assert twin.model is whole.model and twin._t is not whole._t and twin.counter is not whole.counter and twin.chunk is not whole.chunk and twin._packed is not whole._packed
    assert twin.hist is not whole.hist and torch.equal(twin.hist.buf, whole.hist.buf) and torch.equal(twin.hist.len, whole.hist.len)
    assert torch.equal(twin.counter, whole.counter) and torch.equal(twin.chunk, whole.chunk) and int(twin._t) == int(whole._t) == 4
    twin.predict_batch(obs[:, 4])
    assert int(twin._t) == 5 and int(whole._t) == 4 and whole.counter.tolist() == [2, 2, 1] and twin.counter.tolist() == [1, 1, 2] and whole.hist.len.tolist() == [4, 4, 1]
    whole.reset()
    assert whole.counter.tolist() == [c.Ta] * 3 and whole.hist.len.tolist() == [0] * 3
    # emission is the stored chunk row: a lane that is not due ignores its observation, NaN included - but the observation still enters the window
    keep = whole.predict_batch(obs[:, 4])
    stored = whole.chunk.clone()
    again = whole.predict_batch(torch.full_like(obs[:, 5], float("nan")))
    assert torch.equal(again, stored[:, 1]) and torch.equal(keep, stored[:, 0]) and torch.equal(whole.chunk, stored) and not bool(whole.last_bad.any())
    assert whole.hist.len.tolist() == [2] * 3 and bool(torch.isnan(whole.hist.buf[:, -1]).all())
    third = whole.predict_batch(obs[:, 5])      # due, with the NaN row in its window: marked
    assert bool(torch.isnan(third).all()) and whole.last_bad.tolist() == [1, 1, 1]


def test_ragged_batch_equals_per_lane_policies():
    """Lanes with window lengths 1 .. 5 and every counter value in ONE batch against one policy per lane (batch 1), on the Philox stream of the lane's rollout index."""
    c = cfg("a")
    g = torch.Generator().manual_seed(9)
    n = 6
    obs = torch.randn(n, 12, c.OBS, generator=g) * 0.3
    start = [0, 1, 2, 3, 5, 7]      # lane i begins its episode at step start[i]: windows and counters fall out of phase
    batch = golden_policy("a", "cpu", seed=11)
    batch.record = True
    lanes = []
    for i in range(n):
        p = golden_policy("a", "cpu", seed=11)
        p.set_rollout_range(i, 1)
        lanes.append(p)
    seen, widest = set(), 0
    for t in range(12):
        begin = torch.tensor([t == s for s in start])
        if bool(begin.any()):
            batch.begin_episodes(begin)
        a = batch.predict_batch(obs[:, t])
        for i, p in enumerate(lanes):
            if t == start[i]:
                p.begin_episodes(torch.tensor([True]))
            p._t.fill_(t)
            b = p.predict_batch(obs[i:i + 1, t])
            assert int(p.counter) == int(batch.counter[i]) and int(p.hist.len) == int(batch.hist.len[i])
            assert float((a[i] - b[0]).abs().max()) <= 4 * c.D and float((batch.chunk[i] - p.chunk[0]).abs().max()) <= 4 * c.D, (t, i)
        now = {(int(l), int(k)) for l, k in zip(batch.hist.len, batch.counter)}
        seen, widest = seen | now, max(widest, len(now))
    # (window and counter restart together: L = counter up to 4, then L = 5 with every counter) - and one call held five different (L, counter) pairs
    assert seen == {(1, 1), (2, 2), (3, 3), (4, 4), (5, 1), (5, 2), (5, 3), (5, 4)} and widest >= 5


def test_nonfinite_window_row_marks_its_lane_only():
    b = Bank("a")
    clean, dirty = golden_policy("a", "cpu", noise_in=b.noise_in), golden_policy("a", "cpu", noise_in=b.noise_in)
    obs = torch.as_tensor(G["da_a_obs"][:, 0]).clone()
    want = clean.predict_batch(obs)
    for val in (float("nan"), float("inf")):
        dirty.reset()
        bad = obs.clone()
        bad[2, 1] = val
        have = dirty.predict_batch(bad)
        assert torch.isnan(have[2]).all() and torch.isnan(dirty.chunk[2]).all() and dirty.last_bad.tolist() == [0, 0, 1, 0]
        assert torch.equal(have[[0, 1, 3]], want[[0, 1, 3]]) and torch.equal(dirty.chunk[[0, 1, 3]], clean.chunk[[0, 1, 3]])


def test_torch_path_refuses_what_it_cannot_do_and_kernel_shapes():
    pol = golden_policy("a", "cpu")
    assert pol._kernel_shape() and not pol.fused_ok(torch.zeros(1, 10))      # the shipped shape is one the kernel takes; on the CPU the torch path runs
    wide = P.DDPMACTPolicy.random(10, 2, device="cpu", embed_dim=128)
    mlp_head = P.DDPMACTPolicy.random(10, 2, device="cpu", linear_output=False)
    assert not wide._kernel_shape() and not mlp_head._kernel_shape()
    y = mlp_head.predict_batch(torch.zeros(2, 10))
    assert y.shape == (2, 2) and bool(torch.isfinite(y).all())
    with pytest.raises(AssertionError):
        P.pack_ddpm_act_weights(wide.model, 16)


def test_binding_has_the_headers_argument_list():
    """capi's argtypes of d3il_ddpm_act_chunk_f32 against the declaration in include/d3il_rollout.h: count and kind (pointer / float / 64-bit / long / int) of every argument."""
    import ctypes as Ct
    import re
    from d3il_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "d3il_rollout.h")).read()
    decl = re.search(r"int d3il_ddpm_act_chunk_f32\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kind = lambda a: Ct.c_void_p if "*" in a else Ct.c_float if a.startswith("float") else Ct.c_uint64 if a.startswith("uint64_t") else Ct.c_long if a.startswith("long") else Ct.c_int
    assert len(args) == 38
    assert capi.load().d3il_ddpm_act_chunk_f32.argtypes == [kind(a) for a in args]
    assert "d3il_ddpm_act_chunk_f32" in capi.EXPORTS


def test_single_chain_steps_from_the_f64_iterates():
    """Case a per chain step, teacher-forced: one f32 step of the torch path from the reference's f64 iterate against the f64 result of that step, within 4 x the
    deviation of the reference's own f32 step from the same start (the fixture's ``step_dev32``, worst chunk per chain step).  The whole chain meets 4 D anyway
    (above); this pins where along the chain an error would enter."""
    from collections import deque
    c = cfg("a")
    pol = golden_policy("a", "cpu")
    it, dev32, noise = G[c.p + "iter64"], G[c.p + "step_dev32"], torch.as_tensor(G[c.p + "noise"])
    assert it.shape == (int(G[c.p + "computed"].sum()), c.T + 1, c.Ta, c.A) and dev32.shape == (it.shape[0], c.T)
    ch, worst = 0, 0.0
    for e in range(c.n_env):
        ctx = deque(maxlen=c.S)
        for t in range(c.n_steps):
            if e == c.reset_env and t == c.reset_step:
                ctx.clear()
            ctx.append(pol.scaler.scale_input(torch.as_tensor(G[c.p + "obs"][e, t]).reshape(1, -1)))
            if G[c.p + "computed"][e, t]:
                st = torch.stack(tuple(ctx), dim=1)
                assert st.shape[1] == G[c.p + "len"][e, t]
                for i in range(c.T - 1, -1, -1):
                    x = torch.as_tensor(it[ch, c.T - 1 - i], dtype=torch.float32).unsqueeze(0)
                    have = pol._chain_torch(st, noise[e:e + 1, t], x=x, k_start=i, k_stop=i)[2]
                    err = float(np.abs(have[0].double().numpy() - it[ch, c.T - i]).max())
                    worst = max(worst, err / float(dev32[:, i].max()))
                    assert err <= 4 * float(dev32[:, i].max()), (e, t, i)
                ch += 1
    assert ch == it.shape[0]
    print("teacher-forced chain steps of case a: worst %.2f of the reference's own f32 step deviation" % worst)
