"""policies.ACTPolicy on the CPU against the reference's own ActAgent + ActVAE: tests/golden/ref_act_agent.npz holds a scaler, observations, a latent bank and the
reference rolled out batch-1 per environment TWICE - in f32 as shipped and in f64 (tests/golden/gen_act_goldens.py, run where the reference is).  The weights are
not stored: policies.act_synthetic_state rebuilds them and the fixture's checksum proves it.  D = max |f32 - f64| of the reference's own actions is the yardstick;
the replay must stay within 4 D of the f64 table with identical counters, including the reset that lands mid-chunk.  The device replay of the same fixture is
tests/test_gpu_policies_act.py."""
import math
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch.nn import functional as F  # noqa: E402
from d3il_amd import policies as P  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_act_agent.npz"))
OBS, C, HEADS, ENC, DEC, LAT, T, A, SEED, RESET_ENV, RESET_STEP = (int(v) for v in G["act_cfg"])
D = float(G["act_D"])
_SD = None


def golden_sd():
    """The generator's weights, rebuilt (shared by the tests of this module and of the GPU modules; never modified)."""
    global _SD
    if _SD is None:
        _SD = P.act_synthetic_state(P.act_reference_shapes(OBS, A, T, C, ENC, DEC, LAT, 2), SEED)
    return _SD


def golden_policy(dev, seed=0, **kw):
    sc = P.Scaler(G["act_x_mean"], G["act_x_std"], G["act_y_mean"], G["act_y_std"], G["act_y_bounds"], device=dev)
    pol = P.ACTPolicy(P.ActNet(OBS, A, T, C, HEADS, ENC, DEC, LAT).to(dev), sc, seed=seed, **kw)
    pol.load_reference_state_dict({k: torch.as_tensor(v) for k, v in golden_sd().items()})
    return pol


class Bank:
    """latent_in that replays the golden bank of step ``t``."""

    def __init__(self):
        self.t = 0
        self.latent_in = lambda n: G["act_latent"][:n, self.t]


def replay(dev):
    """The golden rollout as ONE batch of 4 lanes on ``dev``: (worst action deviation from the f64 table, worst chunk deviation, counters equal, clamp entries exact, policy)."""
    b = Bank()
    pol = golden_policy(dev, latent_in=b.latent_in)
    pol.record = True
    obs = G["act_obs"]
    lo, hi = G["act_y_bounds"]
    scale64, shift64 = G["act_y_std"] + 1e-12, G["act_y_mean"]
    edge = (pol.lo.cpu() * pol.out_scale.cpu() + pol.out_shift.cpu(), pol.hi.cpu() * pol.out_scale.cpu() + pol.out_shift.cpu())      # a bound through the two f32 operations
    wa = wc = 0.0
    same = exact = True
    n_edge = 0
    for t in range(obs.shape[1]):
        b.t = t
        if t == RESET_STEP:
            mask = torch.zeros(obs.shape[0], dtype=torch.bool)
            mask[RESET_ENV] = True
            pol.begin_episodes(mask.to(dev))
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        wa = max(wa, float(np.abs(a - G["act_ref64"][:, t]).max()))
        same = same and np.array_equal(pol.counter.cpu().numpy().astype(np.int64), G["act_counter"][:, t])
        ch = pol.last_chunk.cpu()
        wc = max(wc, float(np.abs(ch.numpy().astype(np.float64) - G["act_chunks64"][:, t]).max()))
        scaled = (G["act_chunks64"][:, t] - shift64) / scale64
        at_lo, at_hi = torch.as_tensor(scaled <= lo + 1e-9), torch.as_tensor(scaled >= hi - 1e-9)
        n_edge += int(at_lo.sum() + at_hi.sum())
        exact = exact and torch.equal(ch[at_lo], edge[0].expand_as(ch)[at_lo]) and torch.equal(ch[at_hi], edge[1].expand_as(ch)[at_hi])
    return wa, wc, same, exact, n_edge, pol


def test_rebuilt_weights_are_the_generators():
    sd = golden_sd()
    keys = sorted(sd)
    sums = np.array([float(np.asarray(sd[k], dtype=np.float64).sum()) for k in keys])
    assert len(keys) == len(G["act_w_sums"]) and np.array_equal(sums, G["act_w_sums"])
    for (i, j), want in zip(G["act_w_probe_at"], G["act_w_probes"]):
        assert float(sd[keys[int(i)]].reshape(-1)[int(j)]) == float(want)
    used = {k for k in P.ActNet(OBS, A, T, C, HEADS, ENC, DEC, LAT).state_dict()}
    assert used <= set(keys) and sum(sd[k].size for k in used) == 352386      # the parameters used at inference (configs/agents/act_agent.yaml at T = 3, obs 10, A = 2)
    assert all(sd[k].dtype == np.float32 for k in keys)


def test_policy_rows_equal_reference_predict():
    assert float(np.abs(G["act_ref32"] - G["act_ref64"]).max()) == D and G["act_ref64"].shape == (4, 7, A)
    assert G["act_computed"][0].tolist() == [1, 0, 0, 1, 0, 0, 1] and G["act_computed"][RESET_ENV].tolist() == [1, 0, 0, 1, 1, 0, 0]      # three boundaries; the reset lands mid-chunk
    wa, wc, same, exact, n_edge, pol = replay("cpu")
    print("golden replay (cpu): actions %.3e = %.2f D, chunks %.3e = %.2f D (D %.3e); %d chunk entries on a clamp bound" % (wa, wa / D, wc, wc / D, D, n_edge))
    assert same and exact and n_edge > 0
    assert wa <= 4 * D and wc <= 4 * D
    assert int(pol._t) == 7


def formula(sd, state, latent, T_, heads=4):
    """ActVAE.forward without actions written out on the state dict alone, shaped as the reference writes it (masks sliced from T x T triangles, pos_emb[:, :2])."""
    Cw = sd["state_encoder.weight"].shape[0]
    hd = Cw // heads
    lin = lambda x, p: x @ sd[p + ".weight"].T + sd[p + ".bias"]
    ln = lambda x, p: F.layer_norm(x, (Cw,), sd[p + ".weight"], None, 1e-5)
    sp = lambda v: v.view(v.shape[0], -1, heads, hd).transpose(1, 2)
    tri = torch.tril(torch.ones(T_, T_)).view(1, 1, T_, T_)

    def attend(q, k, v, mask):
        att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hd))
        if mask is not None:
            att = att.masked_fill(mask == 0, float("-inf"))
        return torch.softmax(att, dim=-1) @ v

    def block(x, p, cond):
        h = ln(x, p + "ln1")
        L = h.shape[1]
        y = attend(sp(lin(h, p + "attn.query")), sp(lin(h, p + "attn.key")), sp(lin(h, p + "attn.value")), tri[:, :, :L, :L])
        if cond is not None:
            y = y + attend(sp(lin(h, p + "attn.cross_query")), sp(lin(cond, p + "attn.cross_key")), sp(lin(cond, p + "attn.cross_value")), None)
        x = x + lin(y.transpose(1, 2).reshape(x.shape), p + "attn.proj")
        return x + lin(F.gelu(lin(ln(x, p + "ln2"), p + "mlp.0")), p + "mlp.2")

    n = state.shape[0]
    x = torch.cat([(state @ sd["state_encoder.weight"].T).unsqueeze(1), (latent @ sd["latent_out_proj.weight"].T).unsqueeze(1)], dim=1)
    x = x + sd["pos_emb"][:, :x.shape[1]]
    i = 0
    while "encoder.blocks.%d.ln1.weight" % i in sd:
        x = block(x, "encoder.blocks.%d." % i, None)
        i += 1
    enc = ln(x, "encoder.ln")
    y = sd["query_embed.weight"].unsqueeze(0).repeat(n, 1, 1)
    i = 0
    while "decoder.blocks.%d.ln1.weight" % i in sd:
        y = block(y, "decoder.blocks.%d." % i, enc)
        i += 1
    return lin(ln(y, "decoder.ln"), "action_head")


@pytest.mark.parametrize("T_,obs,A_,enc,dec", [(1, 4, 2, 1, 1), (3, 10, 2, 2, 4), (8, 20, 8, 2, 4)])
def test_module_equals_the_reference_shaped_formula_in_f64(T_, obs, A_, enc, dec):
    pol = P.ACTPolicy.random(obs, A_, T_, device="cpu", seed=5, enc_layers=enc, dec_layers=dec)
    tab, pos0 = P.pack_act_weights(pol.model)["tab"], pol.model.pos_emb[0, 0].clone()
    net = pol.model.double()
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    state, latent = torch.randn(5, obs, generator=g, dtype=torch.float64), torch.rand(5, 32, generator=g, dtype=torch.float64)
    want, have = formula(sd, state, latent, T_), net(state, latent)
    assert have.shape == (5, T_, A_) and float((have - want).abs().max()) <= 1e-12 * float(want.abs().max())
    if T_ == 1:      # the quirks of T = 1: pos_emb's single row lands on both tokens, and the 1 x 1 mask hides nothing from the state token
        assert tuple(sd["pos_emb"].shape) == (1, 1, 64)
        assert torch.equal(tab[:64], tab[64:128]) and torch.equal(tab[:64], pos0)
        moved = latent.clone()
        moved[:, 0] += 0.5
        other = net(state, moved)
        assert float((other - have).abs().max()) > 1e-6


def fake_agent(T_=T, obs=OBS, A_=A, **over):
    net = P.ActNet(obs, A_, T_, C, HEADS, ENC, DEC, LAT)
    if T_ == T and obs == OBS and A_ == A:
        net.load_state_dict({k: torch.as_tensor(golden_sd()[k]) for k in net.state_dict()})
    sc = types.SimpleNamespace(x_mean=G["act_x_mean"][:obs], x_std=G["act_x_std"][:obs], y_mean=G["act_y_mean"][:A_], y_std=G["act_y_std"][:A_], y_bounds=G["act_y_bounds"][:, :A_])
    ag = types.SimpleNamespace(model=net, scaler=sc, gc=False, obs_size=1, window_size=T_, action_seq_size=T_, action_counter=T_, predict=lambda s: None, reset=lambda: None)
    for k, v in over.items():
        setattr(ag, k, v)
    return ag


def test_from_reference_and_adapter_selection():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = fake_agent()
    assert P.ACTPolicy.matches(agent) and not P.BeTPolicy.matches(agent) and not P.DDPMGPTPolicy.matches(agent) and not P.IBCPolicy.matches(agent)
    named = fake_agent()
    del named.gc
    named.goal_conditioned = False
    assert P.ACTPolicy.matches(named) and P.ACTPolicy.matches(fake_agent(T_=8, obs=20, A_=8))
    narrow, goal_enc = fake_agent(), fake_agent()
    narrow.model.decoder = P._ActStack(32, 4, DEC, T, True)
    goal_enc.model.goal_encoder = torch.nn.Linear(4, C, bias=False)
    others = {"goal conditioned": fake_agent(gc=True), "obs_size 2": fake_agent(obs_size=2, window_size=T + 1), "differing widths": narrow, "goal encoder": goal_enc,
              "window != chunk": fake_agent(window_size=T + 1)}
    for name, other in others.items():
        assert not P.ACTPolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    pol = as_batched(agent, 4)
    assert isinstance(pol, P.ACTPolicy) and (pol.T, pol.A, pol.obs_dim) == (T, A, OBS) and pol.counter.tolist() == [T] * 4
    # the converted agent replays the golden rows; training-only keys in the state dict are ignored
    b = Bank()
    extra = dict(agent.model.state_dict())
    extra.update({k: torch.as_tensor(v) for k, v in golden_sd().items()})
    agent.model.state_dict = lambda: extra
    pol = P.ACTPolicy.from_reference(agent, latent_in=b.latent_in)
    a = pol.predict_batch(torch.as_tensor(G["act_obs"][:, 0])).numpy().astype(np.float64)
    assert float(np.abs(a - G["act_ref64"][:, 0]).max()) <= 4 * D
    with pytest.raises((AssertionError, RuntimeError)):
        pol.predict_batch(torch.zeros(2, OBS + 1))


def test_fork_ranges_and_episode_masks():
    obs = torch.as_tensor(G["act_obs"])
    whole, part = golden_policy("cpu", seed=5), golden_policy("cpu", seed=5)
    part.set_rollout_range(1, 2)
    assert part.counter.tolist() == [T, T] and part.env_offset == 1
    for s in range(4):
        if s == 2:
            whole.begin_episodes(torch.tensor([False, False, True, False]))
            part.begin_episodes(torch.tensor([False, True]))
        a, b = whole.predict_batch(obs[:, s]), part.predict_batch(obs[1:3, s])
        assert torch.equal(whole.last_latent[1:3], part.last_latent) and torch.equal(whole.counter[1:3], part.counter)
        assert float((a[1:3] - b).abs().max()) <= 4 * D      # (torch's CPU GEMM may round a 4-row and a 2-row batch differently; the draws are identical)
        if s == 0:
            assert np.array_equal(whole.last_latent.numpy(), P.act_latent_uniforms(5, 0, 4, 0))
        if s == 2:      # lane 2 drew at step word 2, the others keep the latent of step word 0
            assert np.array_equal(whole.last_latent[2].numpy(), P.act_latent_uniforms(5, 0, 4, 2)[2]) and np.array_equal(whole.last_latent[0].numpy(), P.act_latent_uniforms(5, 0, 4, 0)[0])
    assert whole.counter.tolist() == [1, 1, 2, 1]
    # fork: network shared; per-lane state, step word and packed buffers its own
    twin = whole.fork()
    assert twin.model is whole.model and twin._t is not whole._t and twin.counter is not whole.counter and twin.chunk is not whole.chunk and twin._packed is not whole._packed
    assert torch.equal(twin.counter, whole.counter) and torch.equal(twin.chunk, whole.chunk) and int(twin._t) == int(whole._t) == 4
    twin.predict_batch(obs[:, 4])
    assert int(twin._t) == 5 and int(whole._t) == 4 and whole.counter.tolist() == [1, 1, 2, 1] and twin.counter.tolist() == [2, 2, 3, 2]
    whole.reset()
    assert whole.counter.tolist() == [T] * 4
    # emission is the stored chunk row: a lane that is not due ignores its observation, NaN included
    keep = whole.predict_batch(obs[:, 5])
    stored = whole.chunk.clone()
    again = whole.predict_batch(torch.full_like(obs[:, 6], float("nan")))
    assert torch.equal(again, stored[:, 1]) and torch.equal(keep, stored[:, 0]) and torch.equal(whole.chunk, stored)


def test_nonfinite_state_marks_its_lane_only():
    b = Bank()
    clean, dirty = golden_policy("cpu", latent_in=b.latent_in), golden_policy("cpu", latent_in=b.latent_in)
    obs = torch.as_tensor(G["act_obs"][:, 0]).clone()
    want = clean.predict_batch(obs)
    for val in (float("nan"), float("inf")):
        dirty.reset()
        bad = obs.clone()
        bad[2, 1] = val
        have = dirty.predict_batch(bad)
        assert torch.isnan(have[2]).all() and torch.isnan(dirty.chunk[2]).all() and torch.equal(have[[0, 1, 3]], want[[0, 1, 3]]) and torch.equal(dirty.chunk[[0, 1, 3]], clean.chunk[[0, 1, 3]])


def test_host_generator():
    """The words are Philox4x32-10 of the stated counters; every counter field changes them; no tag collision; moments over 2^20 uniforms within 5 sigma."""
    seed, off, t = 0x1234567890ABCDEF, (1 << 32) - 3, 7
    w = P.act_latent_words(seed, off, 3, t)
    assert w.shape == (3, 8, 4) and w.dtype == np.uint32
    for n in range(3):
        ge = off + n
        for q in range(8):
            want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x41430000 | q)
            assert [int(x) for x in want] == w[n, q].tolist()
    u = P.act_latent_uniforms(seed, off, 3, t)
    assert u.dtype == np.float32 and u.shape == (3, 32) and u[2, 4 * 5 + 3] == np.float32((int(w[2, 5, 3]) >> 8) / 2.0 ** 24)
    base = P.act_latent_words(seed, 0, 4, t)
    for other in (P.act_latent_words(seed + 1, 0, 4, t), P.act_latent_words(seed, 4, 4, t), P.act_latent_words(seed, 0, 4, t + 1), P.act_latent_words(seed ^ (1 << 40), 0, 4, t),
                  P.act_latent_words(seed, 1 << 32, 4, t)):
        assert not np.isin(other, base).any()
    assert np.array_equal(P.act_latent_words(seed, 1, 3, t), base[1:]) and len({tuple(x) for x in base.reshape(-1, 4)}) == 4 * 8
    tags = {P.ACT_TAG | q for q in range(8)}
    ibc = {P.IBC_TAG | kind << 14 | kk << 8 | s << 2 | q for kind in range(3) for kk in range(64) for s in range(64) for q in range(2)}
    assert P.ACT_TAG == 0x41430000 and 0 not in tags and P.BET_TAG not in tags and not any((tag & 0xFFFF0000) == P.DDPM_GPT_TAG for tag in tags) and not tags & ibc
    from d3il_amd import capi
    assert capi.ACT_TAG == P.ACT_TAG
    uu = np.concatenate([P.act_latent_uniforms(3, 0, 1 << 14, tt).reshape(-1).astype(np.float64) for tt in range(2)])
    m = uu.size
    print("moments over %d uniforms: mean - 1/2 %.3e (bar %.3e), var - 1/12 %.3e (bar %.3e)" % (m, uu.mean() - 0.5, 5 / np.sqrt(12 * m), uu.var() - 1 / 12, 5 / np.sqrt(180 * m)))
    assert m >= 1 << 20 and uu.min() >= 0.0 and uu.max() <= 1 - 2.0 ** -24
    assert abs(uu.mean() - 0.5) < 5 / np.sqrt(12 * m) and abs(uu.var() - 1 / 12) < 5 / np.sqrt(180 * m)


ENC_M, DEC_M = ("query", "key", "value", "proj"), ("query", "key", "value", "cross_query", "cross_key", "cross_value", "proj")


@pytest.mark.parametrize("T_,obs,A_,enc,dec", [(1, 4, 2, 1, 1), (3, 10, 2, 2, 4), (8, 20, 8, 2, 4)])
def test_packer_index_by_index(T_, obs, A_, enc, dec):
    """[To][t][lane (g, i)][r] = W[16 To + i][16 t + 4 g + r] for every matrix, the layer arrays in the order csrc/policy_act.h reads them."""
    pol = P.ACTPolicy.random(obs, A_, T_, device="cpu", seed=3, enc_layers=enc, dec_layers=dec)
    net, pk = pol.model, pol._pack()
    assert pk["w_in"].shape == (4096,) and pk["tab"].shape == (784,) and pk["enc_w"].shape == (enc, 49152) and pk["enc_v"].shape == (enc, 704)
    assert pk["dec_w"].shape == (dec, 61440) and pk["dec_v"].shape == (dec, 896) and pk["head_w"].shape == (1024,) and all(v.dtype == torch.float32 for v in pk.values())
    rng = np.random.default_rng(0)
    at = lambda flat, off, Nt, To, t, g, i, r: float(flat[off + (((To * Nt + t) * 64) + 16 * g + i) * 4 + r])
    for _ in range(150):
        To, t, g, i, r = (int(rng.integers(0, m)) for m in (4, 4, 4, 16, 4))
        row, col = 16 * To + i, 16 * t + 4 * g + r
        if t < 2:
            assert at(pk["w_in"], 0, 2, To, t, g, i, r) == (float(net.state_encoder.weight[row, col]) if col < obs else 0.0)
            assert at(pk["w_in"], 2048, 2, To, t, g, i, r) == float(net.latent_out_proj.weight[row, col])
        if To == 0:
            assert at(pk["head_w"], 0, 4, 0, t, g, i, r) == (float(net.action_head.weight[i, col]) if i < A_ else 0.0)
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
    tab = pk["tab"]
    assert torch.equal(tab[:128].reshape(2, 64), net.pos_emb[0, :2].expand(2, 64)) and torch.equal(tab[128:128 + 64 * T_].reshape(T_, 64), net.query_embed.weight)
    assert float(tab[128 + 64 * T_:640].abs().sum()) == 0.0 and torch.equal(tab[640:704], net.encoder.ln.weight) and torch.equal(tab[704:768], net.decoder.ln.weight)
    assert torch.equal(tab[768:768 + A_], net.action_head.bias) and float(tab[768 + A_:].abs().sum()) == 0.0


def _to_b(X):      # rows [16, F] -> B-operand order [t][lane (g, j)][r] = X[j][16 t + 4 g + r]
    return X.reshape(16, -1, 4, 4).transpose(1, 2, 0, 3).reshape(-1, 64, 4)


def _from_b(Y):     # [To][lane (g, j)][r] (the D registers of the output tiles) -> rows [16, 16 NTo]
    return Y.reshape(-1, 4, 16, 4).transpose(2, 0, 1, 3).reshape(16, -1)


def _lin(flat, off, Nt, NTo, xin, bias=None):
    """act_lin for output tiles 0 .. NTo-1: D[i][j] = sum_k A[i][k] B[k][j] per 16 x 16 x 4 step; lane (g, i) holds A[i][g], lane (g, j) holds B[g][j] and D[4 g + r][j]."""
    wl = flat[off:off + NTo * Nt * 256].reshape(NTo, Nt, 64, 4)
    out = np.zeros((NTo, 64, 4))
    for To in range(NTo):
        Dm = np.zeros((16, 16))
        for t in range(Nt):
            for r in range(4):
                Dm += wl[To, t, :, r].reshape(4, 16).T @ xin[t, :, r].reshape(4, 16)
        for g in range(4):
            out[To, 16 * g:16 * g + 16] = Dm[4 * g:4 * g + 4].T + (0.0 if bias is None else bias[16 * To + 4 * g:16 * To + 4 * g + 4])
    return out


@pytest.mark.parametrize("T_,obs,A_,enc,dec", [(1, 4, 2, 1, 1), (3, 10, 2, 2, 4), (8, 20, 8, 2, 4)])
def test_operand_scheme_reproduces_the_module(T_, obs, A_, enc, dec):
    """csrc/policy_act.h restated tile by tile in f64 NumPy on the packed buffers, for one tile of 16 environments: products through ``_lin``, wave w = output tile
    w = head w, the attention per (environment, head) on the tile's 16 features, LayerNorm on the four tiles of a row.  Equals the module in f64."""
    pol = P.ACTPolicy.random(obs, A_, T_, device="cpu", seed=9, enc_layers=enc, dec_layers=dec)
    pk = {k: v.double().numpy() for k, v in pol._pack().items()}
    g_ = torch.Generator().manual_seed(2)
    state, latent = torch.randn(16, obs, generator=g_, dtype=torch.float64), torch.rand(16, 32, generator=g_, dtype=torch.float64)
    want = pol.model.double()(state, latent).numpy()
    tab = pk["tab"]
    S = np.zeros((16, 32))
    S[:, :obs] = state.numpy()

    def ln(X, wv):
        mean = X.mean(axis=1, keepdims=True)
        return (X - mean) / np.sqrt(((X - mean) ** 2).mean(axis=1, keepdims=True) + 1e-5) * wv

    def heads(X):      # [16, 64] -> [16 env][4 heads (= tiles)][16]
        return X.reshape(16, 4, 16)

    def attend(q, ks, vs):      # q [16, 64]; ks, vs lists of [16, 64]: softmax over the listed keys per (environment, head)
        s = np.stack([(heads(q) * heads(k)).sum(-1) * 0.25 for k in ks], axis=-1)
        p = np.exp(s - s.max(-1, keepdims=True))
        p = p / p.sum(-1, keepdims=True)
        return sum(p[..., i:i + 1] * heads(v) for i, v in enumerate(vs)).reshape(16, 64)

    def mlp(W, V, off_w, off_b, X):
        hid = _lin(W, off_w, 4, 16, _to_b(X), V[off_b:off_b + 256])
        hid = np.asarray(F.gelu(torch.as_tensor(hid)))
        return _from_b(_lin(W, off_w + 16384, 16, 4, hid, V[off_b + 256:off_b + 320]))

    xe = [_from_b(_lin(pk["w_in"], 0, 2, 4, _to_b(S))) + tab[:64], _from_b(_lin(pk["w_in"], 2048, 2, 4, _to_b(latent.numpy()))) + tab[64:128]]
    for l in range(enc):
        W, V = pk["enc_w"][l], pk["enc_v"][l]
        h = [ln(x, V[:64]) for x in xe]
        q, k, v = ([_from_b(_lin(W, 4096 * m, 4, 4, _to_b(x), V[128 + 64 * m:192 + 64 * m])) for x in h] for m in range(3))
        y = [v[0] if T_ >= 2 else attend(q[0], k, v), attend(q[1], k, v)]
        xe = [x + _from_b(_lin(W, 3 * 4096, 4, 4, _to_b(yy), V[320:384])) for x, yy in zip(xe, y)]
        h = [ln(x, V[64:128]) for x in xe]
        xe = [x + mlp(W, V, 4 * 4096, 384, hh) for x, hh in zip(xe, h)]
    eo = [ln(x, tab[640:704]) for x in xe]
    xd = [np.tile(tab[128 + 64 * t:192 + 64 * t], (16, 1)) for t in range(T_)]
    for l in range(dec):
        W, V = pk["dec_w"][l], pk["dec_v"][l]
        h = [ln(x, V[:64]) for x in xd]
        proj = lambda m, rows: [_from_b(_lin(W, 4096 * m, 4, 4, _to_b(x), V[128 + 64 * m:192 + 64 * m])) for x in rows]
        q, k, v, cq, ck, cv = proj(0, h), proj(1, h), proj(2, h), proj(3, h), proj(4, eo), proj(5, eo)
        y = [attend(q[t], k[:t + 1], v[:t + 1]) + attend(cq[t], ck, cv) for t in range(T_)]
        xd = [x + _from_b(_lin(W, 6 * 4096, 4, 4, _to_b(yy), V[512:576])) for x, yy in zip(xd, y)]
        h = [ln(x, V[64:128]) for x in xd]
        xd = [x + mlp(W, V, 7 * 4096, 576, hh) for x, hh in zip(xd, h)]
    out = np.stack([_lin(pk["head_w"], 0, 4, 1, _to_b(ln(x, tab[704:768])), tab[768:784])[0] for x in xd])      # [T][lane (g, j)][r] = component 4 g + r
    have = out.reshape(T_, 4, 16, 4).transpose(2, 0, 1, 3).reshape(16, T_, 16)
    assert float(np.abs(have[:, :, :A_] - want).max()) <= 1e-11 * float(np.abs(want).max()) and float(np.abs(have[:, :, A_:]).max()) == 0.0


def test_binding_has_the_headers_argument_list():
    """capi's argtypes of d3il_act_chunk_f32 against the declaration in include/d3il_rollout.h: count and kind (pointer / float / 64-bit / long / int) of every argument."""
    import ctypes as Ct
    import re
    from d3il_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "d3il_rollout.h")).read()
    decl = re.search(r"int d3il_act_chunk_f32\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kind = lambda a: Ct.c_void_p if "*" in a else Ct.c_float if a.startswith("float") else Ct.c_uint64 if a.startswith("uint64_t") else Ct.c_long if a.startswith("long") else Ct.c_int
    assert len(args) == 30
    assert capi.load().d3il_act_chunk_f32.argtypes == [kind(a) for a in args]
    assert "d3il_act_chunk_f32" in capi.EXPORTS and capi.load().d3il_version() == 2
