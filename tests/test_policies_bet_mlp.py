"""policies.BeTMLPPolicy on the CPU against the reference's own BetMLP_Agent + BeTPolicy + ResidualMLPNetwork + KMeansDiscretizer + Scaler:
tests/golden/ref_bet_mlp_agent.npz holds fixed-seed weights, bin centres, a scaler, a bank of uniforms and the reference rolled out batch-1 per environment TWICE -
in f32 as shipped and in f64 (tests/golden/gen_bet_mlp_goldens.py, run where the reference is).  D = max |f32 - f64| of the reference's own actions is the yardstick:
the replay (torch's layers on the banked uniforms) must draw the golden bin on EVERY row and stay within 4 D of the f64 table.  The device replay of the same
fixture is tests/test_gpu_policies_bet_mlp.py."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from d3il_amd import policies as P  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_bet_mlp_agent.npz"))
OBS, A, HIDDEN, LAYERS, V = (int(v) for v in G["bm_cfg"])
D = float(G["bm_D"][0])


def golden_sd():
    return {k[len("bm_sd__"):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith("bm_sd__")}


class Bank:
    """uniform_fn that replays the golden bank of step ``t`` ([N, T] table)."""

    def __init__(self):
        self.t = 0
        self.fn = lambda n: G["bm_u"][:n, self.t]


def golden_policy(dev, seed=0, uniform_fn=None):
    sc = P.Scaler(G["bm_x_mean"], G["bm_x_std"], G["bm_y_mean"], G["bm_y_std"], G["bm_y_bounds"], device=dev)
    net = P.ResidualMLP(OBS, HIDDEN, LAYERS, V * (1 + A)).to(dev)
    for p in net.parameters():
        p.requires_grad_(False)
    pol = P.BeTMLPPolicy(net, G["bm_centers"], sc, seed=seed, uniform_fn=uniform_fn)
    pol.load_reference_state_dict({k: v.to(dev) for k, v in golden_sd().items()})
    return pol


def replay(dev):
    """Worst deviation of the golden replay on ``dev`` from the f64 table (every row: the bins must be the golden ones), and the policy."""
    b = Bank()
    pol = golden_policy(dev, uniform_fn=b.fn)
    obs = G["bm_obs"]
    worst = 0.0
    for t in range(obs.shape[1]):
        b.t = t
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        assert np.array_equal(pol.last_bins.cpu().numpy(), G["bm_bins"][:, t]), t      # no row is left out
        assert np.array_equal(pol.last_u.cpu().numpy(), G["bm_u"][:, t])
        worst = max(worst, float(np.abs(a - G["bm_ref64"][:, t]).max()))
    return worst, pol


def test_policy_rows_equal_reference_predict():
    assert float(np.abs(G["bm_ref32"] - G["bm_ref64"]).max()) == D and G["bm_ref64"].shape == (6, 4, A) and D > 0
    edge, cdf_dev = G["bm_edge"]
    assert edge == P.BET_MLP_EDGE and cdf_dev < edge / 4      # the golden bins are decided with a margin no f32 softmax reaches
    assert len(np.unique(G["bm_bins"])) > 10
    bins = G["bm_bins"]
    off = G["bm_raw64"][:, :, V:].reshape(6, 4, V, A)[np.arange(6)[:, None], np.arange(4)[None, :], bins]
    v = G["bm_centers"].astype(np.float64)[bins] + off
    lo, hi = G["bm_y_bounds"]
    hit = (v < lo) | (v > hi)
    assert 0 < hit.sum() < hit.size      # some but not all sums reach the action clamp
    worst, pol = replay("cpu")
    print("golden replay (cpu): actions %.3e = %.2f D (D %.3e)" % (worst, worst / D, D))
    assert worst <= 4 * D
    assert int(pol._t) == 4


def test_host_generator():
    """The words are Philox4x32-10 of the stated counters; every counter field changes them; the tag meets no word of the six other streams (pinned here on the
    host); the uniform is the upper 24 bits of word 0."""
    seed, off, t = 0x1234567890ABCDEF, (1 << 32) - 3, 7
    w = P.bet_mlp_words(seed, off, 3, t)
    assert w.shape == (3, 4) and w.dtype == np.uint32 and P.BET_MLP_TAG == 0x424D4C50
    for n in range(3):
        ge = off + n
        want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x424D4C50)
        assert [int(x) for x in want] == w[n].tolist()
    u = P.bet_mlp_uniforms(seed, off, 3, t)
    assert u.dtype == np.float32 and [float(x) for x in u] == [(int(x) >> 8) / 2.0 ** 24 for x in w[:, 0]]
    assert ((u >= 0) & (u <= 1 - 2.0 ** -24)).all()
    base = P.bet_mlp_words(seed, 0, 4, t)
    for other in (P.bet_mlp_words(seed + 1, 0, 4, t), P.bet_mlp_words(seed, 4, 4, t), P.bet_mlp_words(seed, 0, 4, t + 1), P.bet_mlp_words(seed ^ (1 << 40), 0, 4, t),
                  P.bet_mlp_words(seed, 1 << 32, 4, t)):
        assert not np.isin(other, base).any()
    assert np.array_equal(P.bet_mlp_words(seed, 1, 3, t), base[1:])
    # the fourth counter word against every word of the six other streams
    tag = P.BET_MLP_TAG
    ibc = {P.IBC_TAG | kind << 14 | k << 8 | s << 2 | q for kind in range(3) for k in range(64) for s in range(64) for q in range(2)}
    gpt = {P.DDPM_GPT_TAG | k << 8 | j << 1 | q for k in range(256) for j in range(16) for q in range(2)}
    dact = {P.DDPM_ACT_TAG | k << 8 | j << 1 | q for k in range(256) for j in range(128) for q in range(2)}
    small = {P.ACT_TAG | q for q in range(8)} | {P.CVAE_TAG | q for q in range(8)} | {P.BET_TAG, 0}
    assert tag not in ibc and tag not in gpt and tag not in dact and tag not in small
    assert (tag & 0xFFFF0000) not in {x & 0xFFFF0000 for x in (P.BET_TAG, P.DDPM_GPT_TAG, P.IBC_TAG, P.IBC_TAG + 0x10000, P.ACT_TAG, P.CVAE_TAG, P.DDPM_ACT_TAG)}
    assert len({tag, P.BET_TAG, P.DDPM_GPT_TAG, P.IBC_TAG, P.ACT_TAG, P.CVAE_TAG, P.DDPM_ACT_TAG}) == 7
    same_ctr = lambda tg: np.stack(P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, np.arange(4, dtype=np.uint64), 0, t, tg), axis=-1)
    for tg in (0, P.BET_TAG, P.DDPM_GPT_TAG, P.IBC_TAG, P.ACT_TAG, P.CVAE_TAG, P.DDPM_ACT_TAG):
        assert not np.isin(same_ctr(tg), base).any()
    # uniform over 2^16 draws within 5 sigma
    big = P.bet_mlp_uniforms(3, 0, 1 << 16, 0).astype(np.float64)
    assert abs(big.mean() - 0.5) < 5 * np.sqrt(1 / 12 / big.size) and abs(big.var() - 1 / 12) < 5 * np.sqrt(1 / 180 / big.size)


@pytest.mark.parametrize("hidden,blocks,obs,A_", [(128, 3, 4, 2), (256, 1, 20, 3), (128, 0, 28, 8)])
def test_pack_index_by_index(hidden, blocks, obs, A_):
    """w_logit [T][t][lane (g, i)][r] = W[16 T + i][16 t + 4 g + r] for the 64 logit rows, b_logit their bias; w_off / b_off the offset rows as they are; input layer
    and blocks byte for byte what pack_resmlp_weights gives (32 input columns)."""
    pol = P.BeTMLPPolicy.random(obs, A_, device="cpu", seed=3, hidden_dim=hidden, n_blocks=blocks)
    pk = pol._pack()
    lin_in, blks, lin_out = pol.model._parts()
    NT = hidden // 16
    assert set(pk) == {"w_in", "b_in", "w_blk", "b_blk", "n_blocks", "w_logit", "b_logit", "w_off", "b_off"} and pk["n_blocks"] == blocks
    assert pk["w_logit"].shape == (4, NT, 64, 4) and pk["w_logit"].dtype == torch.float32 and pk["w_logit"].is_contiguous()
    W = lin_out.weight
    for T in range(4):
        for t in range(NT):
            for g in range(4):
                for i in range(16):
                    assert torch.equal(pk["w_logit"][T, t, 16 * g + i], W[16 * T + i, 16 * t + 4 * g:16 * t + 4 * g + 4])
    assert torch.equal(pk["b_logit"], lin_out.bias[:64]) and torch.equal(pk["w_off"], W[64:]) and torch.equal(pk["b_off"], lin_out.bias[64:])
    assert pk["w_off"].shape == (64 * A_, hidden) and pk["w_off"].is_contiguous()
    small = types.SimpleNamespace(out_features=2, weight=W[:2], bias=lin_out.bias[:2])
    std = P.pack_resmlp_weights(lin_in, blks, small)
    assert std["w_in"].shape == (NT, 64, 8)
    for k in ("w_in", "b_in", "w_blk", "b_blk"):
        assert torch.equal(pk[k], std[k]), k
    with pytest.raises(AssertionError):
        P.pack_bet_mlp_weights(lin_in, blks, types.SimpleNamespace(out_features=64, in_features=hidden, weight=W[:64], bias=lin_out.bias[:64]))      # no offset rows


@pytest.mark.parametrize("hidden,nb,obs,A_", [(128, 3, 4, 2), (256, 2, 20, 3), (128, 1, 28, 8)])
def test_operand_scheme_reproduces_the_network(hidden, nb, obs, A_):
    """csrc/policy_bet_mlp.h restated tile by tile in f64 NumPy on the packed buffers - D[i][j] = sum_k A[i][k] B[k][j] per 16 x 16 x 4 step, lane (g, i) holds
    A[i][g], lane (g, j) holds B[g][j] and D[4 g + r][j] - for one row tile: the 7-step input layer, the blocks through w_blk, the four logit tiles with their bias
    written to [row][bin], the draw, the offsets of the drawn bin as eight-lane chunked dot products on the final hidden row read back in B-operand order, bias,
    centre, clamp and inverse scaling.  Equals torch's layers in f64."""
    torch.manual_seed(0)
    pol = P.BeTMLPPolicy.random(obs, A_, device="cpu", seed=5, hidden_dim=hidden, n_blocks=nb, action_scale=0.01, bound=1.0)
    pk = {k: (v.double().numpy() if torch.is_tensor(v) else v) for k, v in pol._pack().items()}
    NT = hidden // 16
    s = torch.randn(16, obs, dtype=torch.float64)
    u = torch.rand(16, dtype=torch.float64)
    pol.model.double()
    want, want_bins, want_p = pol._predict_torch(s, u)
    lo, hi = pol.lo.double().numpy(), pol.hi.double().numpy()

    def tile(wt, xin):      # wt [t][lane][r] (one output tile), xin [t][lane][r] -> D regs [lane][r']
        Dm = np.zeros((16, 16))
        for t in range(NT):
            for r in range(4):
                Dm += wt[t, :, r].reshape(4, 16).T @ xin[t, :, r].reshape(4, 16)
        out = np.zeros((64, 4))
        for g in range(4):
            for j in range(16):
                out[16 * g + j] = Dm[4 * g: 4 * g + 4, j]
        return out

    def layer(wl, xin, bias):
        y = np.stack([tile(wl[To], xin) for To in range(NT)])      # [To][lane][r] = B-operand order of the next layer
        for To in range(NT):
            for g in range(4):
                y[To, 16 * g:16 * g + 16] += bias[16 * To + 4 * g: 16 * To + 4 * g + 4]
        return y

    mish = lambda x: torch.nn.functional.mish(torch.as_tensor(x)).numpy()
    R = np.zeros((16, 28)); R[:, :obs] = s.numpy()
    xo = np.zeros((NT, 64, 4))
    for To in range(NT):
        Dm = np.zeros((16, 16))
        for st in range(7):
            Dm += pk["w_in"][To, :, st].reshape(4, 16).T @ np.stack([R[:, 4 * st + g] for g in range(4)])
        for g in range(4):
            for j in range(16):
                xo[To, 16 * g + j] = Dm[4 * g:4 * g + 4, j] + pk["b_in"][16 * To + 4 * g:16 * To + 4 * g + 4]
    assert (pk["w_in"][:, :, 7] == 0).all()      # the eighth column group is padding the kernel never multiplies
    for b in range(nb):
        y = layer(pk["w_blk"][2 * b], mish(xo), pk["b_blk"][2 * b])
        xo = xo + layer(pk["w_blk"][2 * b + 1], mish(y), pk["b_blk"][2 * b + 1])
    lg = np.zeros((16, 64))
    for T in range(4):
        acc = tile(pk["w_logit"][T], xo)
        for g in range(4):
            for j in range(16):
                for r in range(4):
                    lg[j, 16 * T + 4 * g + r] = acc[16 * g + j, r] + pk["b_logit"][16 * T + 4 * g + r]
    have, bins = np.zeros((16, A_)), np.zeros(16, dtype=np.int64)
    sc, sh, cen = pol.out_scale.double().numpy(), pol.out_shift.double().numpy(), pol.centers.double().numpy()
    clamped = 0
    for jr in range(16):
        p = np.exp(lg[jr] - lg[jr].max())
        c = np.cumsum(p)
        bins[jr] = min(int((c <= float(u[jr]) * c[-1]).sum()), 63)
        assert np.allclose(p / c[-1], want_p[jr].numpy(), rtol=1e-12, atol=0)
        for a in range(A_):
            part = 0.0
            for sub in range(8):
                for jj in range(hidden // 32):
                    q = sub + 8 * jj
                    xv = xo[q >> 2, (q & 3) * 16 + jr]      # features 4 q .. 4 q + 3 of row jr
                    part += float(pk["w_off"][bins[jr] * A_ + a, 4 * q:4 * q + 4] @ xv)
            v = cen[bins[jr], a] + (part + pk["b_off"][bins[jr] * A_ + a])
            clamped += int(v < lo[a] or v > hi[a])
            have[jr, a] = min(max(v, lo[a]), hi[a]) * sc[a] + sh[a]
    assert np.array_equal(bins, want_bins.numpy())
    assert 0 < clamped < 16 * A_      # both sides of the clamp are exercised
    err = float(np.abs(have - want.numpy()).max())
    print("operand scheme against torch in f64: %.3e of %.3e; %d of %d sums clamped" % (err, float(want.abs().max()), clamped, 16 * A_))
    assert err <= 1e-12 * float(want.abs().max())


# ---- duck-typed reference agents (class names as in the reference: matches() goes by them)
class _Block(torch.nn.Module):
    def __init__(self, h, act="Mish", use_norm=False, spectral=False):
        super().__init__()
        mk = (lambda: torch.nn.utils.spectral_norm(torch.nn.Linear(h, h))) if spectral else (lambda: torch.nn.Linear(h, h))
        self.l1, self.l2 = mk(), mk()
        self.act, self.use_norm = getattr(torch.nn, act)(), use_norm


class _Net(torch.nn.Module):
    def __init__(self, act="Mish", use_norm=False, spectral=False, block_spectral=False, vocab=V, act_dim=A, first=None):
        super().__init__()
        first = first if first is not None else torch.nn.Linear(OBS, HIDDEN)
        self.layers = torch.nn.ModuleList([torch.nn.utils.spectral_norm(first) if spectral else first] + [_Block(HIDDEN, act, use_norm, block_spectral) for _ in range(LAYERS // 2)]
                                          + [torch.nn.Linear(HIDDEN, vocab * (1 + act_dim))])


class BeTPolicy(torch.nn.Module):      # (the reference's class inside bet_mlp_agent.py has this name)
    def __init__(self, vocab=V, act_dim=A, predict_offsets=True, **kw):
        super().__init__()
        self.model = _Net(vocab=vocab, act_dim=act_dim if predict_offsets else 0, **kw)
        self.vocab_size, self.act_dim, self.predict_offsets = vocab, act_dim, predict_offsets


class BetMLP_Agent:
    def __init__(self, model=None, load=True, centers=None, encoder=None):
        self.model = model or BeTPolicy()
        self.scaler = types.SimpleNamespace(x_mean=torch.as_tensor(G["bm_x_mean"]), x_std=torch.as_tensor(G["bm_x_std"]), y_mean=torch.as_tensor(G["bm_y_mean"]),
                                            y_std=torch.as_tensor(G["bm_y_std"]), y_bounds=G["bm_y_bounds"])
        self.action_ae = types.SimpleNamespace(bin_centers=torch.as_tensor(G["bm_centers"]) if centers is None else centers)
        self.obs_encoding_net = encoder if encoder is not None else torch.nn.Identity()
        self.min_action, self.max_action = torch.as_tensor(G["bm_y_bounds"][0]), torch.as_tensor(G["bm_y_bounds"][1])
        self.window_size = 1
        if load:
            self.model.model.load_state_dict(golden_sd())

    def predict(self, s):
        return np.zeros(A)

    def reset(self):
        pass


class BC_Agent(BetMLP_Agent):
    pass


def _real_bet_agent():
    """A duck-typed BeT_Agent (what BeTPolicy.from_reference reads): the transformer BeT, which must stay BeTPolicy's."""
    trunk = P.MinGPTTrunk(OBS, 32, 1, 4, 5, V, A)
    ag = types.SimpleNamespace(model=types.SimpleNamespace(model=types.SimpleNamespace(model=trunk, n_head=4)),
                               action_ae=types.SimpleNamespace(bin_centers=torch.as_tensor(G["bm_centers"])),
                               scaler=types.SimpleNamespace(x_mean=torch.as_tensor(G["bm_x_mean"]), x_std=torch.as_tensor(G["bm_x_std"]), y_mean=torch.as_tensor(G["bm_y_mean"]),
                                                            y_std=torch.as_tensor(G["bm_y_std"]), y_bounds=G["bm_y_bounds"]),
                               min_action=torch.as_tensor(G["bm_y_bounds"][0]), max_action=torch.as_tensor(G["bm_y_bounds"][1]), window_size=5, predict=lambda s: s)
    return ag


def test_from_reference_and_adapter_selection():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = BetMLP_Agent()
    assert P.BeTMLPPolicy.matches(agent)
    assert not any(c.matches(agent) for c in (P.BeTPolicy, P.CVAEPolicy, P.IBCPolicy, P.ACTPolicy, P.DDPMGPTPolicy, P.DDPMACTPolicy))
    assert P.BeTMLPPolicy.matches(BetMLP_Agent(BeTPolicy(act_dim=8), load=False, centers=torch.zeros(64, 8)))
    others = {"relu": BetMLP_Agent(BeTPolicy(act="ReLU")), "norm": BetMLP_Agent(BeTPolicy(use_norm=True)), "spectral norm": BetMLP_Agent(BeTPolicy(spectral=True), load=False),
              "spectral norm in a block": BetMLP_Agent(BeTPolicy(block_spectral=True), load=False),
              "vocab_size 32": BetMLP_Agent(BeTPolicy(vocab=32), load=False, centers=torch.zeros(32, A)),
              "no offsets": BetMLP_Agent(BeTPolicy(predict_offsets=False), load=False),
              "A = 9": BetMLP_Agent(BeTPolicy(act_dim=9), load=False, centers=torch.zeros(64, 9)),
              "centres of another width": BetMLP_Agent(centers=torch.zeros(64, A + 1)),
              "an observation encoder": BetMLP_Agent(encoder=torch.nn.Linear(OBS, OBS)),
              "another agent class": BC_Agent()}
    for name, other in others.items():
        assert not P.BeTMLPPolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    # a real BeT agent stays BeTPolicy's, and the reverse
    bet = _real_bet_agent()
    assert P.BeTPolicy.matches(bet) and not P.BeTMLPPolicy.matches(bet) and isinstance(as_batched(bet, 2), P.BeTPolicy)
    assert isinstance(as_batched(types.SimpleNamespace(predict=lambda s: s), 2), RowwiseAgent)
    pol = as_batched(agent, 4)
    assert isinstance(pol, P.BeTMLPPolicy) and pol.V == 64 and pol.A == A and pol.obs_dim == OBS
    assert np.array_equal(pol.lo.numpy(), G["bm_y_bounds"][0].astype(np.float32)) and np.array_equal(pol.hi.numpy(), G["bm_y_bounds"][1].astype(np.float32))
    # the converted agent replays the golden rows
    b = Bank()
    pol = P.BeTMLPPolicy.from_reference(agent, uniform_fn=b.fn)
    a = pol.predict_batch(torch.as_tensor(G["bm_obs"][:, 0])).numpy().astype(np.float64)
    assert np.array_equal(pol.last_bins.numpy(), G["bm_bins"][:, 0]) and float(np.abs(a - G["bm_ref64"][:, 0]).max()) <= 4 * D
    # fork: network shared, step word and packed buffers its own, no records
    twin = pol.fork()
    assert twin.model is pol.model and twin._t is not pol._t and int(twin._t) == int(pol._t) == 1 and twin._packed is not pol._packed and twin.last_bins is None
    b.t = 1
    twin.predict_batch(torch.as_tensor(G["bm_obs"][:, 1]))
    assert int(twin._t) == 2 and int(pol._t) == 1
    with pytest.raises((AssertionError, RuntimeError)):
        pol.predict_batch(torch.zeros(2, OBS + 1))


def test_a_rollout_range_is_a_slice_of_the_whole():
    obs = torch.as_tensor(G["bm_obs"])
    whole, part = golden_policy("cpu", seed=5), golden_policy("cpu", seed=5)
    part.set_rollout_range(1, 2)
    twin = whole.fork()
    twin.set_rollout_range(2, 2)
    for s in range(2):
        a, b, c = whole.predict_batch(obs[:, s]), part.predict_batch(obs[1:3, s]), twin.predict_batch(obs[2:4, s])
        assert torch.equal(whole.last_u[1:3], part.last_u) and torch.equal(whole.last_u[2:4], twin.last_u)
        assert np.array_equal(whole.last_u.numpy(), P.bet_mlp_uniforms(5, 0, 6, s))
        # (torch's CPU GEMM may round a 6-row and a 2-row batch differently, by far less than the margin a draw keeps from the edges of its CDF: every row is compared)
        assert torch.equal(whole.last_bins[1:3], part.last_bins) and torch.equal(whole.last_bins[2:4], twin.last_bins)
        assert float((a[1:3] - b).abs().max()) <= 4 * D and float((a[2:4] - c).abs().max()) <= 4 * D
    assert int(whole._t) == int(part._t) == int(twin._t) == 2
    assert len({float(x) for x in whole.last_u}) == 6


def test_nonfinite_inputs_mark_their_environment_only():
    b = Bank()
    clean = golden_policy("cpu", uniform_fn=b.fn)
    obs = torch.as_tensor(G["bm_obs"][:, 0]).clone()
    want = clean.predict_batch(obs)
    want_bins = clean.last_bins.clone()
    assert torch.isfinite(want).all() and (want_bins >= 0).all()
    for bad in (float("nan"), float("inf"), float("-inf")):
        o = obs.clone()
        o[2, 1] = bad
        dirty = golden_policy("cpu", uniform_fn=b.fn)
        have = dirty.predict_batch(o)
        assert torch.isnan(have[2]).all() and torch.equal(have[[0, 1, 3, 4, 5]], want[[0, 1, 3, 4, 5]])
        assert int(dirty.last_bins[2]) == -1 and torch.equal(dirty.last_bins[[0, 1, 3, 4, 5]], want_bins[[0, 1, 3, 4, 5]])
    # a hidden row beyond the f32 range: finite state, Inf / NaN behind the first layer
    o = obs.clone()
    o[4] = 3e37
    dirty = golden_policy("cpu", uniform_fn=b.fn)
    have = dirty.predict_batch(o)
    assert torch.isnan(have[4]).all() and int(dirty.last_bins[4]) == -1 and torch.equal(have[[0, 1, 2, 3, 5]], want[[0, 1, 2, 3, 5]])


def test_the_torch_path_refuses_a_capture_through_the_host_step_word(monkeypatch):
    pol = golden_policy("cpu")
    monkeypatch.setattr(P, "_capturing", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        pol.predict_batch(torch.as_tensor(G["bm_obs"][:, 0]))


def test_binding_has_the_headers_argument_list():
    """capi's argtypes of d3il_bet_mlp_f32 against the declaration in include/d3il_rollout.h: count and kind (pointer / 64-bit / long / int) of every argument."""
    import ctypes as C
    import re
    from d3il_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "d3il_rollout.h")).read()
    decl = re.search(r"int d3il_bet_mlp_f32\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kind = lambda a: C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_uint64 if a.startswith("uint64_t") else C.c_long if a.startswith("long") else C.c_int
    assert len(args) == 29
    assert [a.split()[-1].lstrip("*") for a in args] == ["state", "w_in", "b_in", "w_blocks", "b_blocks", "w_logit", "b_logit", "w_off", "b_off", "centers", "lo", "hi", "scale", "shift",
                                                         "seed", "env_offset", "t_device", "u_in", "actions", "bins", "u_out", "probs", "n_env", "obs_dim", "V", "A", "hidden",
                                                         "n_blocks", "stream"]
    assert capi.load().d3il_bet_mlp_f32.argtypes == [kind(a) for a in args]
    assert "d3il_bet_mlp_f32" in capi.EXPORTS and capi.BET_MLP_TAG == P.BET_MLP_TAG
    src = open(os.path.join(root, "d3il_amd", "csrc", "policy_bet_mlp.h")).read()
    assert "BET_MLP_TAG = 0x%08Xu" % P.BET_MLP_TAG in src
    assert capi.load().d3il_version() == 2
