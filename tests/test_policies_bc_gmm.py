"""policies.BCGMMPolicy on the CPU against the reference's own BC_GMM + ResidualMLPNetwork + Scaler under BC_Agent.predict: tests/golden/ref_bc_gmm_agent.npz holds,
for three cases, fixed-seed weights, a scaler, a bank of uniforms and normals and the reference rolled out batch-1 per environment TWICE - in f32 as shipped and in
f64 (tests/golden/gen_bc_gmm_goldens.py, run where the reference is).  D = max |f32 - f64| of the reference's own actions, per case, is the yardstick: the replay
(torch's layers on the banked draws) must draw the golden component on EVERY row and stay within 4 D of the f64 table.  The device replay of the same fixture is
tests/test_gpu_policies_bc_gmm.py."""
import copy
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from d3il_amd import policies as P  # noqa: E402
from tests import bc_gmm_cases as B  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_bc_gmm_agent.npz"))
NAMES = ("a", "b", "c")


def cfg(name):
    obs, A, Gn, hidden, layers, act, low = (int(v) for v in G["gm_%s_cfg" % name])
    return dict(obs=obs, A=A, G=Gn, hidden=hidden, layers=layers, std_activation={1: "exp", 2: "softplus"}[act], low_noise_eval=bool(low), min_std=float(G["gm_%s_min_std" % name][0]),
                D=float(G["gm_%s_D" % name][0]))


def golden_sd(name):
    pre = "gm_%s_sd__" % name
    return {k[len(pre):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith(pre)}


class Bank:
    """u_in / z_in that replay the golden bank of step ``t``."""

    def __init__(self, name):
        self.t = 0
        self.u = lambda n: G["gm_%s_u" % name][:n, self.t]
        self.z = lambda n: G["gm_%s_z" % name][:n, self.t]


def golden_policy(name, dev="cpu", seed=0, bank=None):
    c = cfg(name)
    sd = {k: v.to(dev) for k, v in golden_sd(name).items()}
    return P.BCGMMPolicy.from_model(sd, types.SimpleNamespace(**{k: torch.as_tensor(G["gm_%s_%s" % (name, k)]) for k in ("x_mean", "x_std", "y_mean", "y_std", "y_bounds")}),
                                    c["min_std"], c["std_activation"], c["low_noise_eval"], seed=seed, device=dev, u_in=None if bank is None else bank.u,
                                    z_in=None if bank is None else bank.z)


def replay(name, dev):
    """Worst deviation of the golden replay on ``dev`` from the f64 table (every row: the components must be the golden ones), and the policy."""
    b = Bank(name)
    pol = golden_policy(name, dev, bank=b)
    obs = G["gm_%s_obs" % name]
    worst = 0.0
    for t in range(obs.shape[1]):
        b.t = t
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        assert np.array_equal(pol.last_comps.cpu().numpy(), G["gm_%s_comps" % name][:, t]), t      # no row is left out
        assert np.array_equal(pol.last_u.cpu().numpy(), G["gm_%s_u" % name][:, t]) and np.array_equal(pol.last_z.cpu().numpy(), G["gm_%s_z" % name][:, t])
        worst = max(worst, float(np.abs(a - G["gm_%s_ref64" % name][:, t]).max()))
    return worst, pol


@pytest.mark.parametrize("name", NAMES)
def test_policy_rows_equal_reference_predict(name):
    c = cfg(name)
    ref32, ref64 = G["gm_%s_ref32" % name], G["gm_%s_ref64" % name]
    assert float(np.abs(ref32 - ref64).max()) == c["D"] and ref64.shape == (6, 4, c["A"]) and c["D"] > 0
    edge, cdf_dev = G["gm_%s_edge" % name]
    assert edge == P.BC_GMM_EDGE and cdf_dev < edge / 4      # the golden components are decided with a margin no f32 softmax reaches
    if name == "b":
        lo, hi = G["gm_b_y_bounds"]
        hit = (G["gm_b_x64"] < lo) | (G["gm_b_x64"] > hi)
        assert 0 < hit.sum() < hit.size      # some but not all samples reach the action clamp
    worst, pol = replay(name, "cpu")
    print("golden replay %s (cpu): actions %.3e = %.2f D (D %.3e)" % (name, worst, worst / c["D"], c["D"]))
    assert worst <= 4 * c["D"]
    assert int(pol._t) == 4 and (pol.G, pol.A, pol.obs_dim) == (c["G"], c["A"], c["obs"])
    assert pol._kernel_shape() == (name != "b")      # (b) is the torch path's case


def test_host_generator():
    """The words are Philox4x32-10 of the stated counters; every counter field changes them; the tag's upper half is no other tag's; the uniform is the upper 24 bits
    of word 0 of call 0, the normals are Box-Muller on calls 1 and 2, component a = 4 (q - 1) + m."""
    seed, off, t = 0x1234567890ABCDEF, (1 << 32) - 3, 7
    w = P.bc_gmm_words(seed, off, 3, t)
    assert w.shape == (3, 3, 4) and w.dtype == np.uint32 and P.BC_GMM_TAG == 0x474D0000
    for n in range(3):
        ge = off + n
        for q in range(3):
            want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x474D0000 | q)
            assert [int(x) for x in want] == w[n, q].tolist()
    u = P.bc_gmm_uniforms(seed, off, 3, t)
    assert u.dtype == np.float32 and [float(x) for x in u] == [(int(x) >> 8) / 2.0 ** 24 for x in w[:, 0, 0]]
    z = P.bc_gmm_normals(seed, off, 3, t, 8)
    assert z.shape == (3, 8) and z.dtype == np.float64
    for n in range(3):
        for a in range(8):
            r = w[n, 1 + a // 4]
            pair = (a % 4) // 2
            u1, u2 = ((int(r[2 * pair]) >> 8) + 1) * 2.0 ** -24, (int(r[2 * pair + 1]) >> 8) * 2.0 ** -24
            want = np.sqrt(-2.0 * np.log(u1)) * (np.sin if a % 2 else np.cos)(2.0 * np.pi * u2)
            assert abs(z[n, a] - want) <= 1e-15 * max(1.0, abs(want))
    assert np.array_equal(P.bc_gmm_normals(seed, off, 3, t, 3), z[:, :3])
    base = P.bc_gmm_words(seed, 0, 4, t)
    for other in (P.bc_gmm_words(seed + 1, 0, 4, t), P.bc_gmm_words(seed, 4, 4, t), P.bc_gmm_words(seed, 0, 4, t + 1), P.bc_gmm_words(seed ^ (1 << 40), 0, 4, t),
                  P.bc_gmm_words(seed, 1 << 32, 4, t)):
        assert not np.isin(other, base).any()
    assert np.array_equal(P.bc_gmm_words(seed, 1, 3, t), base[1:])
    # the upper half of the tag against every other tag's (the layout bits of every stream live in the lower half; IBC's reach one bit into the upper)
    from d3il_amd import capi
    others = (P.BET_TAG, P.DDPM_GPT_TAG, P.IBC_TAG, P.IBC_TAG + 0x10000, P.ACT_TAG, P.CVAE_TAG, P.DDPM_ACT_TAG, P.BET_MLP_TAG, P.BESO_TAG, P.DDPM_MLP_TAG, 0)
    assert P.BC_GMM_TAG >> 16 not in {x >> 16 for x in others} and P.BC_GMM_TAG & 0xFFFF == 0
    assert capi.TAG_BC_GMM == P.BC_GMM_TAG
    # moments over 2^16 draws within 5 sigma
    big = P.bc_gmm_uniforms(3, 0, 1 << 16, 0).astype(np.float64)
    assert abs(big.mean() - 0.5) < 5 * np.sqrt(1 / 12 / big.size) and abs(big.var() - 1 / 12) < 5 * np.sqrt(1 / 180 / big.size)
    zz = P.bc_gmm_normals(3, 0, 1 << 16, 0, 8).reshape(-1)
    assert abs(zz.mean()) < 5 / np.sqrt(zz.size) and abs(zz.var() - 1) < 5 * np.sqrt(2 / zz.size)


def test_the_device_drawn_launch_leaves_few_rows_out():
    """The constants of the GPU test's device-drawn launch, on the host: the f64 restatement alone puts DRAWN_NEAR <= DRAWN_CAP of the 257 rows within EDGE of an edge."""
    c, u, z, (y, k, p), near = B.drawn_reference()
    assert int(near.sum()) == B.DRAWN_NEAR <= B.DRAWN_CAP and c.G == 64
    assert torch.isfinite(y).all() and len(set(k.tolist())) > 32


@pytest.mark.parametrize("hidden,blocks,obs,A_,Gn", [(128, 3, 4, 2, 8), (256, 1, 20, 3, 17), (128, 0, 28, 8, 64), (128, 1, 1, 1, 1)])
def test_pack_index_by_index(hidden, blocks, obs, A_, Gn):
    """w_feat [T][t][lane (g, i)][r] = W_o[16 T + i][16 t + 4 g + r]; w_logit the same order on the G logit rows padded to 64 with zeros; the mean and std rows as
    they are; input layer and blocks byte for byte what pack_resmlp_weights gives (32 input columns)."""
    pol = P.BCGMMPolicy.random(obs, A_, device="cpu", seed=3, hidden_dim=hidden, n_blocks=blocks, n_gaussians=Gn)
    pk = pol._pack()
    net = pol.model
    lin_in, blks, lin_out = net.mlp._parts()
    NT = hidden // 16
    assert set(pk) == {"w_in", "b_in", "w_blk", "b_blk", "n_blocks", "w_feat", "b_feat", "w_logit", "b_logit", "w_mean", "b_mean", "w_std", "b_std"} and pk["n_blocks"] == blocks
    assert pk["w_feat"].shape == (NT, NT, 64, 4) and pk["w_logit"].shape == (4, NT, 64, 4) and all(pk[k].dtype == torch.float32 and pk[k].is_contiguous() for k in pk if k != "n_blocks")
    Wl = torch.zeros(64, hidden)
    Wl[:Gn] = net.logits_mlp.weight
    for packed, W, tiles in ((pk["w_feat"], lin_out.weight, NT), (pk["w_logit"], Wl, 4)):
        for T in range(tiles):
            for t in range(NT):
                for g in range(4):
                    for i in range(16):
                        assert torch.equal(packed[T, t, 16 * g + i], W[16 * T + i, 16 * t + 4 * g:16 * t + 4 * g + 4])
    assert torch.equal(pk["b_feat"], lin_out.bias) and torch.equal(pk["b_logit"][:Gn], net.logits_mlp.bias) and not pk["b_logit"][Gn:].any() and pk["b_logit"].shape == (64,)
    assert torch.equal(pk["w_mean"], net.mean_mlp.weight) and torch.equal(pk["b_mean"], net.mean_mlp.bias) and pk["w_mean"].shape == (Gn * A_, hidden)
    assert torch.equal(pk["w_std"], net.std_mlp.weight) and torch.equal(pk["b_std"], net.std_mlp.bias)
    std = P.pack_resmlp_weights(lin_in, blks, types.SimpleNamespace(out_features=2, weight=lin_out.weight[:2], bias=lin_out.bias[:2]))
    for k in ("w_in", "b_in", "w_blk", "b_blk"):
        assert torch.equal(pk[k], std[k]), k


def test_packed_tables_follow_the_parameters():
    """PackedWeights through load_state_dict, use_ema and invalidate_packed: the tables are the current parameters' after each, in the same buffers."""
    pol = P.BCGMMPolicy.random(4, 2, device="cpu", seed=3, hidden_dim=128, n_blocks=1, n_gaussians=8)
    tables = lambda: (pol._packed.ensure(pol._pack_params(), pol._pack), pol._packed.buf)[1]
    first = tables()
    key = pol._packed.key
    assert tables() is first and pol._packed.key == key      # nothing changed: nothing packed
    other = P.BCGMMPolicy.random(4, 2, device="cpu", seed=4, hidden_dim=128, n_blocks=1, n_gaussians=8)
    pol.load_reference_state_dict(other.model.state_dict())
    second = tables()
    assert second is first and pol._packed.key != key      # refreshed in place: a captured graph keeps reading them
    assert torch.equal(second["w_mean"], other.model.mean_mlp.weight) and torch.equal(second["w_feat"], other._pack()["w_feat"])
    pol.use_ema([p.detach() * 0.5 for p in pol.model.parameters()])
    third = tables()
    assert torch.equal(third["w_mean"], other.model.mean_mlp.weight * 0.5) and torch.equal(third["b_logit"][:8], other.model.logits_mlp.bias * 0.5)
    pol.model.std_mlp.weight.data.mul_(2.0)      # invisible to the version counters
    assert torch.equal(tables()["w_std"], other.model.std_mlp.weight * 0.5)      # (stale)
    pol.invalidate_packed()
    assert torch.equal(tables()["w_std"], other.model.std_mlp.weight)


# ---- duck-typed reference agents (class names and attribute names as in the reference: matches() goes by them)
class _Block(torch.nn.Module):
    def __init__(self, h, act="Mish", use_norm=False, spectral=False):
        super().__init__()
        mk = (lambda: torch.nn.utils.spectral_norm(torch.nn.Linear(h, h))) if spectral else (lambda: torch.nn.Linear(h, h))
        self.l1, self.l2 = mk(), mk()
        self.act, self.use_norm = getattr(torch.nn, act)(), use_norm


class _Net(torch.nn.Module):
    def __init__(self, obs, hidden, layers, out_dim, act="Mish", use_norm=False, spectral=False):
        super().__init__()
        first = torch.nn.Linear(obs, hidden)
        self.layers = torch.nn.ModuleList([torch.nn.utils.spectral_norm(first) if spectral else first] + [_Block(hidden, act, use_norm) for _ in range(layers // 2)]
                                          + [torch.nn.Linear(hidden, out_dim)])


class BC_GMM(torch.nn.Module):
    def __init__(self, obs=4, hidden=128, layers=2, A=2, Gn=8, act="Mish", mlp_output_dim=None, std_activation="exp", tanh_wrapped=False, low_noise_eval=True, **kw):
        super().__init__()
        out = hidden if mlp_output_dim is None else mlp_output_dim
        self.mlp = _Net(obs, hidden, layers, out, act=act, **kw)
        self.mlp_output_act = getattr(torch.nn, act)()
        self.mean_mlp, self.std_mlp, self.logits_mlp = torch.nn.Linear(out, A * Gn), torch.nn.Linear(out, A * Gn), torch.nn.Linear(out, Gn)
        self.output_dim, self.n_gaussians, self.min_std, self.std_activation = A, Gn, 1e-4, std_activation
        self.use_tanh_wrapped_distribution, self.low_noise_eval = tanh_wrapped, low_noise_eval
        self.eval()


class BC_GMM_Agent:
    def __init__(self, model=None, load=True, bounds=True):
        self.model = model or BC_GMM()
        g = lambda k: torch.as_tensor(G["gm_a_" + k])
        self.scaler = types.SimpleNamespace(x_mean=g("x_mean"), x_std=g("x_std"), y_mean=g("y_mean"), y_std=g("y_std"), y_bounds=G["gm_a_y_bounds"] if bounds else None)
        self.min_action, self.max_action = g("y_bounds")[0], g("y_bounds")[1]
        if load:
            self.model.load_state_dict(golden_sd("a"))

    def predict(self, s):
        return np.zeros(self.model.output_dim)

    def reset(self):
        pass


class BC_Agent(BC_GMM_Agent):
    pass


def test_from_reference_and_adapter_selection():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = BC_GMM_Agent()
    assert P.BCGMMPolicy.matches(agent)
    rest = (P.BeTPolicy, P.BeTMLPPolicy, P.GPTBCPolicy, P.CVAEPolicy, P.IBCPolicy, P.ACTPolicy, P.DDPMGPTPolicy, P.DDPMACTPolicy, P.DDPMNativePolicy, P.BESONativePolicy)
    assert not any(c.matches(agent) for c in rest)      # no other policy's matches accepts it
    assert P.BCGMMPolicy.matches(BC_GMM_Agent(BC_GMM(A=8, Gn=64, std_activation="softplus", low_noise_eval=False), load=False))
    train = BC_GMM_Agent()
    train.model.train()
    others = {"tanh-wrapped distribution": BC_GMM_Agent(BC_GMM(tanh_wrapped=True)), "another std activation": BC_GMM_Agent(BC_GMM(std_activation="relu")), "train mode": train,
              "norm": BC_GMM_Agent(BC_GMM(use_norm=True)), "spectral norm": BC_GMM_Agent(BC_GMM(spectral=True), load=False), "another activation": BC_GMM_Agent(BC_GMM(act="ReLU")),
              "G = 65": BC_GMM_Agent(BC_GMM(Gn=65), load=False), "A = 9": BC_GMM_Agent(BC_GMM(A=9), load=False),
              "mlp_output_dim != hidden_dim": BC_GMM_Agent(BC_GMM(mlp_output_dim=64), load=False), "a missing scaler bound": BC_GMM_Agent(bounds=False),
              "another agent class": BC_Agent()}
    for name, other in others.items():
        assert not P.BCGMMPolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    assert isinstance(as_batched(types.SimpleNamespace(predict=lambda s: s), 2), RowwiseAgent)
    pol = as_batched(agent, 4)
    c = cfg("a")
    assert isinstance(pol, P.BCGMMPolicy) and (pol.G, pol.A, pol.obs_dim) == (c["G"], c["A"], c["obs"]) and pol.low_noise_eval and pol.std_mode == 0 and pol.min_std == 1e-4
    assert np.array_equal(pol.lo.numpy(), G["gm_a_y_bounds"][0].astype(np.float32)) and np.array_equal(pol.hi.numpy(), G["gm_a_y_bounds"][1].astype(np.float32))
    # the converted agent replays the golden rows
    b = Bank("a")
    pol = P.BCGMMPolicy.from_reference(agent, u_in=b.u, z_in=b.z)
    a = pol.predict_batch(torch.as_tensor(G["gm_a_obs"][:, 0])).numpy().astype(np.float64)
    assert np.array_equal(pol.last_comps.numpy(), G["gm_a_comps"][:, 0]) and float(np.abs(a - G["gm_a_ref64"][:, 0]).max()) <= 4 * c["D"]
    # fork: network shared, step word and packed buffers its own, no records
    twin = pol.fork()
    assert twin.model is pol.model and twin._t is not pol._t and int(twin._t) == int(pol._t) == 1 and twin._packed is not pol._packed and twin.last_comps is None and twin.last_z is None
    b.t = 1
    twin.predict_batch(torch.as_tensor(G["gm_a_obs"][:, 1]))
    assert int(twin._t) == 2 and int(pol._t) == 1
    with pytest.raises((AssertionError, RuntimeError)):
        pol.predict_batch(torch.zeros(2, c["obs"] + 1))


@pytest.mark.parametrize("name", ["a", "c"])
def test_a_rollout_range_is_a_slice_of_the_whole(name):
    obs = torch.as_tensor(G["gm_%s_obs" % name])
    c = cfg(name)
    whole, part = golden_policy(name, seed=(5 << 32) + 9), golden_policy(name, seed=(5 << 32) + 9)
    part.set_rollout_range(1, 2)
    twin = whole.fork()
    twin.set_rollout_range(2, 2)
    for s in range(2):
        a, b, d = whole.predict_batch(obs[:, s]), part.predict_batch(obs[1:3, s]), twin.predict_batch(obs[2:4, s])
        assert torch.equal(whole.last_u[1:3], part.last_u) and torch.equal(whole.last_u[2:4], twin.last_u)      # bit for bit
        assert torch.equal(whole.last_z[1:3], part.last_z) and torch.equal(whole.last_z[2:4], twin.last_z)
        assert np.array_equal(whole.last_u.numpy(), P.bc_gmm_uniforms((5 << 32) + 9, 0, 6, s))
        assert np.array_equal(whole.last_z.numpy(), P.bc_gmm_normals((5 << 32) + 9, 0, 6, s, c["A"]).astype(np.float32))
        # (torch's CPU GEMM may round a 6-row and a 2-row batch differently: the rows whose u keeps EDGE from the edges of its CDF are compared - here all of them)
        assert torch.equal(whole.last_comps[1:3], part.last_comps) and torch.equal(whole.last_comps[2:4], twin.last_comps)
        assert float((a[1:3] - b).abs().max()) <= 4 * c["D"] and float((a[2:4] - d).abs().max()) <= 4 * c["D"]
    assert int(whole._t) == int(part._t) == int(twin._t) == 2      # forks have their own step words
    twin.predict_batch(obs[2:4, 2])
    assert int(twin._t) == 3 and int(whole._t) == 2
    assert len({float(x) for x in whole.last_u}) == 6


@pytest.mark.parametrize("name", ["a", "b"])
def test_nonfinite_values_mark_their_environment_only(name):
    b = Bank(name)
    clean = golden_policy(name, bank=b)
    obs = torch.as_tensor(G["gm_%s_obs" % name][:, 0]).clone()
    want = clean.predict_batch(obs)
    want_k = clean.last_comps.clone()
    rest = [0, 1, 3, 4, 5]
    assert torch.isfinite(want).all() and (want_k >= 0).all()
    for bad in (float("nan"), float("inf"), float("-inf")):
        o = obs.clone()
        o[2, 1] = bad
        dirty = golden_policy(name, bank=b)
        have = dirty.predict_batch(o)
        assert torch.isnan(have[2]).all() and torch.equal(have[rest], want[rest])
        assert int(dirty.last_comps[2]) == -1 and torch.equal(dirty.last_comps[rest], want_k[rest])
        # a used draw
        zb = G["gm_%s_z" % name][:, 0].copy()
        zb[2, -1] = bad
        dirty = golden_policy(name, bank=b)
        dirty.z_in = lambda n: zb[:n]
        have = dirty.predict_batch(obs)
        assert torch.isnan(have[2]).all() and torch.equal(have[rest], want[rest]) and int(dirty.last_comps[2]) == -1
    # a feature row beyond the f32 range: finite state, Inf / NaN behind the first layer
    o = obs.clone()
    o[4] = 3e37
    dirty = golden_policy(name, bank=b)
    have = dirty.predict_batch(o)
    assert torch.isnan(have[4]).all() and int(dirty.last_comps[4]) == -1 and torch.equal(have[[0, 1, 2, 3, 5]], want[[0, 1, 2, 3, 5]])


def test_an_overflowing_exp_std_marks_its_environment():
    """std = exp(raw) = Inf: the clamp would turn mean + Inf z into a bound; the row is marked instead."""
    b = Bank("b")
    pol = golden_policy("b", bank=b)
    pol.model = copy.deepcopy(pol.model)
    obs = torch.as_tensor(G["gm_b_obs"][:, 0])
    want = pol.predict_batch(obs).clone()
    with torch.no_grad():
        pol.model.std_mlp.bias[int(G["gm_b_comps"][3, 0]) * pol.A + 1] = 100.0      # exp(100) overflows f32; only rows that draw this component read it
    have = pol.predict_batch(obs)
    hit = [r for r in range(6) if int(G["gm_b_comps"][r, 0]) == int(G["gm_b_comps"][3, 0])]
    good = [r for r in range(6) if r not in hit]
    assert 3 in hit and torch.isnan(have[hit]).all() and (pol.last_comps[hit] == -1).all() and torch.equal(have[good], want[good])


def test_softplus_is_torchs():
    """The identity above 20 (torch's threshold), log1p(exp(x)) below: the policy calls F.softplus itself; the kernel restates the switch."""
    x = torch.tensor([-5.0, 0.0, 19.999, 20.0, 20.001, 50.0])
    assert torch.equal(torch.nn.functional.softplus(x), torch.where(x > 20.0, x, torch.log1p(torch.exp(x))))
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "d3il_amd", "csrc", "policy_bc_gmm.h")).read()
    assert "sraw > 20.f ? sraw : log1pf(expf(sraw))" in src and "BC_GMM_TAG = 0x%08Xu" % P.BC_GMM_TAG in src


def test_the_torch_path_refuses_a_capture_through_the_host_step_word(monkeypatch):
    pol = golden_policy("a")
    monkeypatch.setattr(P, "_capturing", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        pol.predict_batch(torch.as_tensor(G["gm_a_obs"][:, 0]))


def test_random_policy_has_spread_logits():
    pol = P.BCGMMPolicy.random(4, 2, device="cpu", seed=1, n_gaussians=64, low_noise_eval=False)
    pol.record = True
    y = pol.predict_batch(torch.randn(512, 4, generator=torch.Generator().manual_seed(2)))
    logits = pol.last_probs.log()
    assert torch.isfinite(y).all() and 1.0 < float(logits.std(dim=1).mean()) < 3.0 and len(set(pol.last_comps.tolist())) > 32
    assert pol.SWITCH == "D3IL_POLICY_BC_GMM_FUSED"
