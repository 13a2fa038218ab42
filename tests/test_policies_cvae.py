"""policies.CVAEPolicy on the CPU against the reference's own CVAEAgent + VariationalAE + ResidualMLPNetwork + Scaler: tests/golden/ref_cvae_agent.npz holds
fixed-seed decoder weights, a scaler, a bank of unclamped prior samples and the reference rolled out batch-1 per environment TWICE - in f32 as shipped and in f64
(tests/golden/gen_cvae_goldens.py, run where the reference is).  D = max |f32 - f64| of the reference's own actions is the yardstick; the replay (torch's layers on
the banked latent) must stay within 4 D of the f64 table.  The device replay of the same fixture is tests/test_gpu_policies_cvae.py."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from d3il_amd import policies as P  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cvae_agent.npz"))
OBS, A, HIDDEN, LAYERS, L = (int(v) for v in G["cvae_cfg"])
D = float(G["cvae_D"][0])


def golden_sd(prefix=""):
    return {prefix + k[len("cvae_sd__"):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith("cvae_sd__")}


class Bank:
    """z_in that replays the golden bank of step ``t`` ([N, T, L] table of unclamped normals)."""

    def __init__(self):
        self.t = 0
        self.z_in = lambda n: G["cvae_z"][:n, self.t]


def golden_policy(dev, seed=0, z_in=None):
    sc = P.Scaler(G["cvae_x_mean"], G["cvae_x_std"], G["cvae_y_mean"], G["cvae_y_std"], G["cvae_y_bounds"], device=dev)
    net = P.ResidualMLP(OBS + L, HIDDEN, LAYERS, A).to(dev)
    for p in net.parameters():
        p.requires_grad_(False)
    pol = P.CVAEPolicy(net, sc, L, seed=seed, z_in=z_in)
    pol.load_reference_state_dict(golden_sd("decoder."))
    return pol


def replay(dev):
    """Worst deviation of the golden replay on ``dev`` from the f64 table, and the policy."""
    b = Bank()
    pol = golden_policy(dev, z_in=b.z_in)
    obs = G["cvae_obs"]
    worst = 0.0
    for t in range(obs.shape[1]):
        b.t = t
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(a - G["cvae_ref64"][:, t]).max()))
        assert np.array_equal(pol.last_z.cpu().numpy().astype(np.float64), G["cvae_in64"][:, t, OBS:])      # the clamped latent the reference's decoder saw
    return worst, pol


def test_policy_rows_equal_reference_predict():
    assert float(np.abs(G["cvae_ref32"] - G["cvae_ref64"]).max()) == D and G["cvae_ref64"].shape == (4, 4, A) and D > 0
    lo, hi = G["cvae_y_bounds"]
    hit = (G["cvae_raw64"] < lo) | (G["cvae_raw64"] > hi)
    assert 0 < hit.sum() < hit.size      # some but not all outputs reach the action clamp
    assert np.array_equal(G["cvae_in64"][:, :, OBS:], np.clip(G["cvae_z"].astype(np.float64), -0.5, 0.5))      # state first, the clamped latent second
    worst, pol = replay("cpu")
    print("golden replay (cpu): actions %.3e = %.2f D (D %.3e)" % (worst, worst / D, D))
    assert worst <= 4 * D
    assert int(pol._t) == 4


def test_host_generator():
    """The words are Philox4x32-10 of the stated counters; every counter field changes them; the tag meets none of the five others; moments over 2^20 normals and
    the share of components the +-0.5 clamp moves within 5 sigma."""
    seed, off, t = 0x1234567890ABCDEF, (1 << 32) - 3, 7
    w = P.cvae_words(seed, off, 3, t)
    assert w.shape == (3, 8, 4) and w.dtype == np.uint32 and P.CVAE_TAG == 0x43560000
    for n in range(3):
        ge = off + n
        for q in range(8):
            want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x43560000 | q)
            assert [int(x) for x in want] == w[n, q].tolist()
    z = P.cvae_latent_normals(seed, off, 3, t, 32)
    assert z.shape == (3, 32) and z.dtype == np.float64
    r = w[1, 5].astype(np.float64)
    u1, u2 = (np.floor(r[2] / 256) + 1) / 2 ** 24, np.floor(r[3] / 256) / 2 ** 24
    assert z[1, 22] == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2) and z[1, 23] == np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)
    u1, u2 = (np.floor(r[0] / 256) + 1) / 2 ** 24, np.floor(r[1] / 256) / 2 ** 24
    assert z[1, 20] == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2) and z[1, 21] == np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)
    for LL in (1, 16, 24):
        assert np.array_equal(P.cvae_latent_normals(seed, off, 3, t, LL), z[:, :LL])
    # every field of the counter matters, and no two (row, q) share a word
    base = P.cvae_words(seed, 0, 4, t)
    for other in (P.cvae_words(seed + 1, 0, 4, t), P.cvae_words(seed, 4, 4, t), P.cvae_words(seed, 0, 4, t + 1), P.cvae_words(seed ^ (1 << 40), 0, 4, t),
                  P.cvae_words(seed, 1 << 32, 4, t)):
        assert not np.isin(other, base).any()
    assert np.array_equal(P.cvae_words(seed, 1, 3, t), base[1:])
    assert len({tuple(x) for x in base.reshape(-1, 4)}) == 4 * 8
    # the fourth counter words against those of the five other streams
    tags = {P.CVAE_TAG | q for q in range(8)}
    ibc = {P.IBC_TAG | kind << 14 | k << 8 | s << 2 | q for kind in range(3) for k in range(64) for s in range(64) for q in range(2)}
    gpt = {P.DDPM_GPT_TAG | k << 8 | j << 1 | q for k in range(256) for j in range(16) for q in range(2)}
    act = {P.ACT_TAG | q for q in range(8)}
    assert 0 not in tags and P.BET_TAG not in tags and not (tags & ibc) and not (tags & gpt) and not (tags & act) and len(tags) == 8
    assert not any((tg & 0xFFFF0000) in (P.DDPM_GPT_TAG, P.IBC_TAG, P.IBC_TAG + 0x10000, P.ACT_TAG) for tg in tags)
    # the rollout's words differ from the other policies' words at the same (seed, row, t)
    same_ctr = lambda tag: np.stack(P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, np.arange(4, dtype=np.uint64), 0, t, tag), axis=-1)
    for tag in (0, P.BET_TAG, P.DDPM_GPT_TAG, P.IBC_TAG, P.ACT_TAG):
        assert not np.isin(same_ctr(tag), base).any()
    # moments over 2^20 normals; the clamp moves 2 (1 - Phi(0.5)) of them
    big = P.cvae_latent_normals(3, 0, 1 << 15, 0, 32).reshape(-1)
    n = big.size
    p = 0.6170750774519738      # erfc(0.5 / sqrt(2))
    moved = float((np.abs(big) > 0.5).mean())
    print("moments over %d normals: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e); clamped share %.5f (p %.5f, bar %.2e)"
          % (n, big.mean(), 5 / np.sqrt(n), big.var() - 1, 5 * np.sqrt(2 / n), moved, p, 5 * np.sqrt(p * (1 - p) / n)))
    assert n == 1 << 20 and np.isfinite(big).all()
    assert abs(big.mean()) < 5 / np.sqrt(n) and abs(big.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs(moved - p) < 5 * np.sqrt(p * (1 - p) / n)
    import math
    assert abs(p - math.erfc(0.5 / math.sqrt(2))) < 1e-15 and round(p, 5) == 0.61708


@pytest.mark.parametrize("hidden,blocks,obs,L_,A_", [(128, 3, 4, 32, 2), (256, 1, 20, 16, 8), (128, 0, 32, 32, 16), (128, 1, 22, 24, 2)])
def test_input_layer_packs_to_64_columns(hidden, blocks, obs, L_, A_):
    """w_in [T_out][lane (g, i)][s] = W[16 T_out + i][4 s + g] for s < 16, zero beyond the decoder's input width; the rest is pack_resmlp_weights' default."""
    pol = P.CVAEPolicy.random(obs, A_, device="cpu", seed=3, hidden_dim=hidden, n_blocks=blocks, latent_dim=L_)
    pk = pol._pack()
    lin_in, blks, lin_out = pol.model._parts()
    NT, IN = hidden // 16, obs + L_
    assert pk["w_in"].shape == (NT, 64, 16) and pk["w_in"].dtype == torch.float32 and pk["n_blocks"] == blocks
    W = lin_in.weight
    for To in range(NT):
        for g in range(4):
            for i in range(16):
                for s in range(16):
                    want = float(W[16 * To + i, 4 * s + g]) if 4 * s + g < IN else 0.0
                    assert float(pk["w_in"][To, 16 * g + i, s]) == want
    std = P.pack_resmlp_weights(lin_in, blks, lin_out) if IN <= 32 else None
    narrow = std if std is not None else P.pack_resmlp_weights(types.SimpleNamespace(weight=W[:, :32], bias=lin_in.bias, in_features=32, out_features=hidden), blks, lin_out)
    assert torch.equal(pk["w_in"][:, :, :8], narrow["w_in"])
    for k in ("b_in", "w_blk", "b_blk", "w_out", "b_out"):
        assert torch.equal(pk[k], narrow[k]), k
    with pytest.raises(AssertionError):
        P.pack_resmlp_weights(types.SimpleNamespace(weight=torch.zeros(hidden, 65), bias=lin_in.bias, in_features=65, out_features=hidden), blks, lin_out, in_cols=64)


@pytest.mark.parametrize("hidden,nb,obs,L_,A_", [(128, 3, 4, 32, 2), (256, 2, 20, 16, 8), (128, 1, 32, 32, 16)])
def test_operand_scheme_reproduces_the_decoder(hidden, nb, obs, L_, A_):
    """csrc/policy_cvae.h restated tile by tile in f64 NumPy on the packed buffers - D[i][j] = sum_k A[i][k] B[k][j] per 16 x 16 x 4 step, lane (g, i) holds A[i][g],
    lane (g, j) holds B[g][j] and D[4 g + r][j] - for one row tile: the 16-step input layer on [state | clamped latent] with its two accumulators, the blocks
    through w_blk, the output tile, bias, clamp and inverse scaling read from lane (g, j), register r = component 4 g + r.  Equals torch's layers in f64."""
    torch.manual_seed(0)
    pol = P.CVAEPolicy.random(obs, A_, device="cpu", hidden_dim=hidden, n_blocks=nb, latent_dim=L_, weight_gain=1.6, action_scale=0.01, bound=0.5)
    pk = {k: (v.double().numpy() if torch.is_tensor(v) else v) for k, v in pol._pack().items()}
    NT, IN = hidden // 16, obs + L_
    s = torch.randn(16, obs, dtype=torch.float64)
    z = torch.randn(16, L_, dtype=torch.float64)
    pol.model.double()
    want, zc = pol._decode_torch(s, z)
    raw = torch.cat([s, zc], dim=1)
    for layer in pol.model.layers:
        raw = layer(raw)
    lo, hi = pol.lo.double().numpy(), pol.hi.double().numpy()
    assert ((raw.numpy() < lo) | (raw.numpy() > hi)).any() and ((raw.numpy() > lo) & (raw.numpy() < hi)).any()      # both sides of the clamp are exercised

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
    # input row: in_k[s] of lane (g, j) = feature 4 s + g of row j = state for f < obs, clamped latent f - obs for f < obs + L, zero beyond
    R = np.zeros((16, 64)); R[:, :obs] = s.numpy(); R[:, obs:IN] = np.clip(z.numpy(), -0.5, 0.5)
    xo = np.zeros((NT, 64, 4))
    for To in range(NT):
        acc, acc2 = np.zeros((16, 16)), np.zeros((16, 16))
        for st in range(16):
            Amat = pk["w_in"][To, :, st].reshape(4, 16)
            Bmat = np.stack([R[:, 4 * st + g] for g in range(4)])
            if st % 2 == 0:
                acc += Amat.T @ Bmat
            else:
                acc2 += Amat.T @ Bmat
        Dm = acc + acc2
        for g in range(4):
            for j in range(16):
                xo[To, 16 * g + j] = Dm[4 * g:4 * g + 4, j] + pk["b_in"][16 * To + 4 * g:16 * To + 4 * g + 4]
    for b in range(nb):
        u = layer(pk["w_blk"][2 * b], mish(xo), pk["b_blk"][2 * b])
        xo = xo + layer(pk["w_blk"][2 * b + 1], mish(u), pk["b_blk"][2 * b + 1])
    acc = tile(pk["w_out"], xo)
    have = np.zeros((16, A_))
    sc, sh = pol.out_scale.double().numpy(), pol.out_shift.double().numpy()
    for g in range(4):
        for j in range(16):
            for r in range(4):
                c = 4 * g + r
                if c < A_:
                    have[j, c] = min(max(acc[16 * g + j, r] + pk["b_out"][c], lo[c]), hi[c]) * sc[c] + sh[c]
                else:
                    assert acc[16 * g + j, r] == 0.0 and pk["b_out"][c] == 0.0
    err = float(np.abs(have - want.numpy()).max())
    print("operand scheme against torch in f64: %.3e of %.3e" % (err, float(want.abs().max())))
    assert err <= 1e-12 * float(want.abs().max())


# ---- duck-typed reference agents (class names as in the reference: matches() goes by them)
class _Block(torch.nn.Module):
    def __init__(self, h, act="Mish", use_norm=False, spectral=False):
        super().__init__()
        mk = (lambda: torch.nn.utils.spectral_norm(torch.nn.Linear(h, h))) if spectral else (lambda: torch.nn.Linear(h, h))
        self.l1, self.l2 = mk(), mk()
        self.act, self.use_norm = getattr(torch.nn, act)(), use_norm


class _Net(torch.nn.Module):
    def __init__(self, act="Mish", use_norm=False, spectral=False, in_dim=OBS + L, first=None, block_spectral=False):
        super().__init__()
        first = first if first is not None else torch.nn.Linear(in_dim, HIDDEN)
        self.layers = torch.nn.ModuleList([torch.nn.utils.spectral_norm(first) if spectral else first] + [_Block(HIDDEN, act, use_norm, block_spectral) for _ in range(LAYERS // 2)]
                                          + [torch.nn.Linear(HIDDEN, A)])


class VariationalAE(torch.nn.Module):
    def __init__(self, latent_dim=L, **kw):
        super().__init__()
        self.decoder = _Net(**kw)
        self.encoder = torch.nn.Linear(3, 3)      # never read at evaluation
        self.latent_dim = latent_dim


class OtherAE(VariationalAE):
    pass


class CVAEAgent:
    def __init__(self, model=None, load=True):
        self.model = model or VariationalAE()
        self.scaler = types.SimpleNamespace(x_mean=torch.as_tensor(G["cvae_x_mean"]), x_std=torch.as_tensor(G["cvae_x_std"]), y_mean=torch.as_tensor(G["cvae_y_mean"]),
                                            y_std=torch.as_tensor(G["cvae_y_std"]), y_bounds=G["cvae_y_bounds"])
        if load:
            self.model.decoder.load_state_dict(golden_sd())

    def predict(self, s):
        return np.zeros(A)

    def reset(self):
        pass


class BC_Agent(CVAEAgent):
    pass


class _Gated(torch.nn.Linear):      # a layer that is a Linear by inheritance only
    pass


def test_from_reference_and_adapter_selection():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = CVAEAgent()
    assert P.CVAEPolicy.matches(agent) and not P.IBCPolicy.matches(agent) and not P.BeTPolicy.matches(agent) and not P.ACTPolicy.matches(agent) and not P.DDPMGPTPolicy.matches(agent)
    assert P.CVAEPolicy.matches(CVAEAgent(VariationalAE(latent_dim=32, in_dim=64), load=False))      # the widest input row
    assert P.CVAEPolicy.matches(CVAEAgent(VariationalAE(latent_dim=1, in_dim=2), load=False))
    others = {"relu": CVAEAgent(VariationalAE(act="ReLU")), "norm": CVAEAgent(VariationalAE(use_norm=True)), "spectral norm": CVAEAgent(VariationalAE(spectral=True), load=False),
              "spectral norm in a block": CVAEAgent(VariationalAE(block_spectral=True), load=False),
              "a layer that is not a plain Linear": CVAEAgent(VariationalAE(first=_Gated(OBS + L, HIDDEN))), "a convolution": CVAEAgent(VariationalAE(first=torch.nn.Conv1d(OBS + L, HIDDEN, 1)), load=False),
              "latent 33": CVAEAgent(VariationalAE(latent_dim=33, in_dim=OBS + 33), load=False), "obs + latent 65": CVAEAgent(VariationalAE(latent_dim=32, in_dim=65), load=False),
              "no state": CVAEAgent(VariationalAE(latent_dim=L, in_dim=L), load=False), "another model class": CVAEAgent(OtherAE()), "another agent class": BC_Agent()}
    for name, other in others.items():
        assert not P.CVAEPolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    assert isinstance(as_batched(types.SimpleNamespace(predict=lambda s: s), 2), RowwiseAgent)
    pol = as_batched(agent, 4)
    assert isinstance(pol, P.CVAEPolicy) and pol.L == L and pol.A == A and pol.obs_dim == OBS and pol.n_envs == 4
    assert not any(k.startswith("encoder") for k in pol.model.state_dict())
    assert np.array_equal(pol.lo.numpy(), G["cvae_y_bounds"][0].astype(np.float32)) and np.array_equal(pol.hi.numpy(), G["cvae_y_bounds"][1].astype(np.float32))
    # the converted agent replays the golden rows
    b = Bank()
    pol = P.CVAEPolicy.from_reference(agent, z_in=b.z_in)
    a = pol.predict_batch(torch.as_tensor(G["cvae_obs"][:, 0])).numpy().astype(np.float64)
    assert float(np.abs(a - G["cvae_ref64"][:, 0]).max()) <= 4 * D
    # fork: network shared, step word and packed buffers its own
    twin = pol.fork()
    assert twin.model is pol.model and twin._t is not pol._t and int(twin._t) == int(pol._t) == 1 and twin._packed is not pol._packed
    twin.predict_batch(torch.as_tensor(G["cvae_obs"][:, 1]))
    assert int(twin._t) == 2 and int(pol._t) == 1
    with pytest.raises((AssertionError, RuntimeError)):
        pol.predict_batch(torch.zeros(2, OBS + 1))
    # load_reference_state_dict takes the whole VariationalAE state and ignores the encoder
    fresh = golden_policy("cpu")
    with torch.no_grad():
        for p in fresh.model.parameters():
            p.zero_()
    fresh.load_reference_state_dict(agent.model.state_dict())
    assert all(torch.equal(v, golden_sd()[k]) for k, v in fresh.model.state_dict().items())


def test_a_rollout_range_is_a_slice_of_the_whole():
    obs = torch.as_tensor(G["cvae_obs"])
    whole, part = golden_policy("cpu", seed=5), golden_policy("cpu", seed=5)
    part.set_rollout_range(1, 2)
    twin = whole.fork()
    twin.set_rollout_range(2, 2)
    for s in range(2):
        a, b, c = whole.predict_batch(obs[:, s]), part.predict_batch(obs[1:3, s]), twin.predict_batch(obs[2:4, s])
        assert torch.equal(whole.last_z[1:3], part.last_z) and torch.equal(whole.last_z[2:4], twin.last_z)
        want = np.clip(P.cvae_latent_normals(5, 0, 4, s, L).astype(np.float32), np.float32(-0.5), np.float32(0.5))
        assert np.array_equal(whole.last_z.numpy(), want)
        # (torch's CPU GEMM may round a 4-row and a 2-row batch differently; the draws are identical)
        assert float((a[1:3] - b).abs().max()) <= 4 * D and float((a[2:4] - c).abs().max()) <= 4 * D
    assert int(whole._t) == int(part._t) == int(twin._t) == 2
    assert float((whole.last_z.abs() == 0.5).float().mean()) > 0.3


def test_nonfinite_inputs_mark_their_environment_only():
    b = Bank()
    clean = golden_policy("cpu", z_in=b.z_in)
    obs = torch.as_tensor(G["cvae_obs"][:, 0]).clone()
    want = clean.predict_batch(obs)
    assert torch.isfinite(want).all()
    for bad_obs, bad_z in ((float("nan"), None), (float("inf"), None), (None, float("nan")), (None, float("-inf"))):
        zb = G["cvae_z"][:, 0].copy()
        o = obs.clone()
        if bad_obs is not None:
            o[2, 1] = bad_obs
        else:
            zb[2, 3] = bad_z
        dirty = golden_policy("cpu", z_in=lambda n: zb[:n])
        have = dirty.predict_batch(o)
        assert torch.isnan(have[2]).all() and torch.equal(have[[0, 1, 3]], want[[0, 1, 3]])


def test_binding_has_the_headers_argument_list():
    """capi's argtypes of d3il_cvae_decode_f32 against the declaration in include/d3il_rollout.h: count and kind (pointer / 64-bit / long / int) of every argument."""
    import ctypes as C
    import re
    from d3il_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "d3il_rollout.h")).read()
    decl = re.search(r"int d3il_cvae_decode_f32\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kind = lambda a: C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_uint64 if a.startswith("uint64_t") else C.c_long if a.startswith("long") else C.c_int
    assert len(args) == 24
    assert [a.split()[-1].lstrip("*") for a in args] == ["state", "w_in", "b_in", "w_blocks", "b_blocks", "w_out", "b_out", "lo", "hi", "scale", "shift", "seed", "env_offset", "t_device",
                                                         "z_in", "actions", "z_out", "n_env", "obs_dim", "latent", "A", "hidden", "n_blocks", "stream"]
    assert capi.load().d3il_cvae_decode_f32.argtypes == [kind(a) for a in args]
    assert "d3il_cvae_decode_f32" in capi.EXPORTS and capi.CVAE_TAG == P.CVAE_TAG
    assert capi.load().d3il_version() == 2
