"""policies.DDPMNativePolicy on the CPU against the reference's own DiffusionAgent + Diffusion + DiffusionMLPNetwork: tests/golden/ref_ddpm_mlp_agent.npz holds, for
three cases (a: avoiding shape, a kernel shape; b: aligning shape, T = 24; c: stacking shape at window 5), fixed-seed weights, scaler statistics, observations, one
banked normal per (environment, step, call, position, component) and the reference's actions, rolled out batch-1 per environment TWICE - in f32 as shipped and in
f64 (tests/golden/gen_ddpm_mlp_goldens.py, run where the reference is; case c with the one repair its docstring describes).  D = max |f32 - f64| of the reference
itself, per case, is the yardstick: the replay has to stay within 4 D of the f64 table on every row (the chain is continuous in its inputs: no row is left out).  The
gpu-marked replay of the same fixture is tests/test_gpu_policies_ddpm_mlp.py."""
import os
import types

import numpy as np
import pytest
import torch
from torch import nn

from d3il_amd import capi
from d3il_amd import policies as P

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ddpm_mlp_agent.npz"))
CASES = ("a", "b", "c")


def cfg(c):
    """(obs, A, t_dim, T, window, hidden, hidden layers) of case c."""
    return tuple(int(v) for v in G[c + "_cfg"])


def golden_sd(c):
    pre = c + "_sd__"
    return {k[len(pre):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith(pre)}


def golden_scaler(c, dev):
    return P.Scaler(G[c + "_x_mean"], G[c + "_x_std"], G[c + "_y_mean"], G[c + "_y_std"], G[c + "_y_bounds"], device=dev)


class Bank:
    """noise_in that replays table[:, call, k] ([n, calls, T + 1, A]: the newest window position of the fixture's bank); a predict call starts with draw 0."""

    def __init__(self, table):
        self.table, self.call = torch.as_tensor(table, dtype=torch.float32), -1

    def __call__(self, k, n):
        if k == 0:
            self.call += 1
        return self.table[:n, self.call, k]


def golden_policy(c, dev, noise_in=None, seed=0, window=None):
    OBS, A, TD, T, W, HID, NHID = cfg(c)
    pol = P.DDPMNativePolicy(P.DiffusionMLP(A, OBS, TD, HID, NHID).to(dev), golden_scaler(c, dev), T, W if window is None else window, seed=seed, noise_in=noise_in)
    pol.load_reference_state_dict(golden_sd(c))
    return pol


def replay(c, dev, window=None):
    """(worst |action - f64 table|, worst |action - f32 table|, policy, actions [6, 8, A]) of the golden replay of case c on ``dev``, all 48 rows."""
    pol = golden_policy(c, dev, Bank(G[c + "_noise"][:, :, :, -1]), window=window)
    obs = G[c + "_obs"]
    acts = np.stack([pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64) for t in range(obs.shape[1])], axis=1)
    return float(np.abs(acts - G[c + "_ref64"]).max()), float(np.abs(acts - G[c + "_ref32"]).max()), pol, acts


# ------------------------------------------------------------------------------------------------ golden replay, window independence
@pytest.mark.parametrize("c", CASES)
def test_policy_rows_equal_reference_predict(c):
    D = float(G[c + "_D"])
    assert float(np.abs(G[c + "_ref32"] - G[c + "_ref64"]).max()) == D and G[c + "_ref64"].shape == (6, 8, cfg(c)[1])
    w64, w32, pol, _ = replay(c, "cpu")
    print("golden replay (cpu), case %s: D %.3e, worst |action - f64 reference| %.3e (%.2f D), worst |action - f32 reference| %.3e" % (c, D, w64, w64 / D, w32))
    assert w64 <= 4 * D
    assert int(pol._t) == 8 and pol.last_bad.tolist() == [0] * 6 and pol.hist is None
    assert pol._kernel_shape() == (c == "a")


def test_the_cases_are_the_shapes_they_are_meant_to_be():
    assert cfg("a") == (4, 2, 24, 4, 1, 128, 2) and cfg("b") == (20, 3, 8, 24, 1, 32, 4) and cfg("c") == (20, 8, 4, 4, 5, 32, 4)
    for c in CASES:
        OBS, A, TD, T, W, HID, NHID = cfg(c)
        assert G[c + "_noise"].shape == (6, 8, T + 1, W, A) and G[c + "_obs"].shape == (6, 8, OBS)
        assert all(k.startswith("model.") for k in golden_sd(c))
        res = P.DiffusionMLP(A, OBS, TD, HID, NHID).load_state_dict({k[len("model."):]: v for k, v in golden_sd(c).items()})
        assert not res.missing_keys and not res.unexpected_keys


def test_window_five_equals_window_one():
    """Case c: the reference ran it at window 5; the policy keeps no history, so window_size 5 and window_size 1 give the same actions - bit for bit -, reset and
    begin_episodes change nothing, and both meet the reference's table."""
    D = float(G["c_D"])
    w5, _, pol5, a5 = replay("c", "cpu")
    w1, _, pol1, a1 = replay("c", "cpu", window=1)
    assert pol5.W == 5 and pol1.W == 1 and np.array_equal(a5, a1) and w5 <= 4 * D and w1 <= 4 * D
    pol = golden_policy("c", "cpu", Bank(G["c_noise"][:, :, :, -1]))
    obs = torch.as_tensor(G["c_obs"])
    first = pol.predict_batch(obs[:, 0]).clone()
    pol.reset()
    pol.begin_episodes(torch.ones(6, dtype=torch.uint8))
    second = pol.predict_batch(obs[:, 1])
    assert np.array_equal(first.numpy().astype(np.float64), a5[:, 0]) and np.array_equal(second.numpy().astype(np.float64), a5[:, 1])


# ------------------------------------------------------------------------------------------------ routing
class _RefBlock(nn.Module):
    """The attributes of the reference's TwoLayerPreActivationResNetLinear (mlp.py:9-46) that ``matches`` reads."""

    def __init__(self, h, p=0.0):
        super().__init__()
        self.l1, self.l2, self.dropout, self.use_norm, self.act = nn.Linear(h, h), nn.Linear(h, h), nn.Dropout(p), False, nn.Mish()

    def forward(self, x):
        return x + self.l2(self.act(self.l1(self.act(x))))


class _RefDenoiser(nn.Module):
    """A module with the attribute and parameter names of the reference's DiffusionMLPNetwork (diffusion_models.py:20-118), residual style."""

    def __init__(self, A, obs, t_dim, hid, n_hidden):
        super().__init__()
        self.temp_layers = nn.Sequential(P._SinusoidalPosEmb(t_dim), nn.Linear(t_dim, 2 * t_dim), nn.Mish(), nn.Linear(2 * t_dim, t_dim))
        self.layers = nn.Module()
        self.layers.layers = nn.ModuleList([nn.Linear(A + t_dim + obs, hid)] + [_RefBlock(hid) for _ in range(n_hidden // 2)] + [nn.Linear(hid, A)])
        self.goal_conditioned = False


def _stand_in_agent(c="a", use_ema=False):
    """An object with the attributes from_reference reads off a live DiffusionAgent around a DiffusionMLPNetwork, carrying the fixture's tensors."""
    OBS, A, TD, T, W, HID, NHID = cfg(c)
    net = _RefDenoiser(A, OBS, TD, HID, NHID)
    res = net.load_state_dict({k[len("model."):]: v for k, v in golden_sd(c).items()})
    assert not res.missing_keys and not res.unexpected_keys
    f64 = lambda k: torch.as_tensor(G[c + k], dtype=torch.float64)
    scaler = types.SimpleNamespace(x_mean=f64("_x_mean"), x_std=f64("_x_std"), y_mean=f64("_y_mean"), y_std=f64("_y_std"), y_bounds=G[c + "_y_bounds"])
    shadow = [p.detach().clone() + 0.01 for p in net.parameters()]
    diff = types.SimpleNamespace(model=net, n_timesteps=T, betas=P.cosine_beta_schedule(T), predict_epsilon=True, clip_denoised=True, diffusion_x=False)
    return types.SimpleNamespace(model=diff, scaler=scaler, window_size=W, use_ema=use_ema, diffusion_kde=False, ema_helper=types.SimpleNamespace(shadow_params=shadow),
                                 predict=lambda s: (_ for _ in ()).throw(AssertionError("the batched policy must not call predict")))


@pytest.mark.parametrize("c", CASES)
def test_from_reference_and_adapter_selection(c):
    from d3il_amd.agents import as_batched
    OBS, A, TD, T, W, HID, NHID = cfg(c)
    agent = _stand_in_agent(c)
    assert P.DDPMNativePolicy.matches(agent) and not P.DDPMGPTPolicy.matches(agent) and not P.DDPMACTPolicy.matches(agent)
    assert not any(cls.matches(agent) for cls in (P.BeTPolicy, P.BESONativePolicy, P.IBCPolicy, P.ACTPolicy, P.CVAEPolicy, P.BeTMLPPolicy, P.GPTBCPolicy))
    pol = as_batched(agent, 6)
    assert isinstance(pol, P.DDPMNativePolicy) and (pol.T, pol.W, pol.A, pol.t_dim, pol.obs_dim) == (T, W, A, TD, OBS) and pol.model is not agent.model.model
    assert len(pol.model.layers.layers) == NHID // 2 + 2 and pol.model.layers.layers[0].out_features == HID
    pol.noise_in = Bank(G[c + "_noise"][:, :, :, -1])
    for t in range(3):
        a = pol.predict_batch(torch.as_tensor(G[c + "_obs"][:, t]))
        assert float(np.abs(a.numpy().astype(np.float64) - G[c + "_ref64"][:, t]).max()) <= 4 * float(G[c + "_D"])


def test_every_other_sampler_switch_stays_row_by_row():
    from d3il_amd.agents import RowwiseAgent, as_batched
    T, A = cfg("a")[3], cfg("a")[1]
    for where, name, value in (("model", "diffusion_x", True), ("agent", "diffusion_kde", True), ("model", "predict_epsilon", False), ("model", "clip_denoised", False),
                               ("model", "betas", torch.linspace(1e-4, 2e-2, T)), ("model", "betas", P.cosine_beta_schedule(T + 1)), ("net", "goal_conditioned", True),
                               ("model", "n_timesteps", 256)):
        other = _stand_in_agent()
        setattr({"model": other.model, "agent": other, "net": other.model.model}[where], name, value)
        other.predict = lambda s_: np.zeros((1, A))
        assert not P.DDPMNativePolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    no_betas = _stand_in_agent(); del no_betas.model.betas
    no_betas.predict = lambda s_: np.zeros((1, A))
    assert not P.DDPMNativePolicy.matches(no_betas) and isinstance(as_batched(no_betas, 2), RowwiseAgent)
    no_scaler = _stand_in_agent(); del no_scaler.scaler
    assert not P.DDPMNativePolicy.matches(no_scaler)
    # what the restated network does not have: norm, dropout, spectral norm (weight_orig), another activation, a transformer denoiser's attributes
    for change in ("use_norm", "dropout", "act", "weight_orig", "time_emb", "blocks", "encoder"):
        other = _stand_in_agent()
        net = other.model.model
        blk = net.layers.layers[1]
        if change == "use_norm":
            blk.use_norm = True
        elif change == "dropout":
            blk.dropout = nn.Dropout(0.1)
        elif change == "act":
            blk.act = nn.ReLU()
        elif change == "weight_orig":
            blk.l1.weight_orig = blk.l1.weight
        else:
            setattr(net, change, nn.Identity())
        assert not P.DDPMNativePolicy.matches(other), change
    # the stand-in of tests/test_policies_ddpm_gpt.py (the project's own DiffusionMLP, no betas) keeps failing every matches
    mlp_agent = types.SimpleNamespace(model=types.SimpleNamespace(model=P.DiffusionMLP(2, 16, 8, 32, 4), n_timesteps=4), scaler=_stand_in_agent().scaler, window_size=1, predict=lambda s: s)
    assert not P.DDPMNativePolicy.matches(mlp_agent) and isinstance(as_batched(mlp_agent, 2), RowwiseAgent)


def test_use_ema_swaps_the_shadow_parameters_in():
    from d3il_amd.agents import as_batched
    plain, ema = as_batched(_stand_in_agent(), 6), as_batched(_stand_in_agent(use_ema=True), 6)
    for p, q in zip(plain.model.parameters(), ema.model.parameters()):
        assert torch.equal(q, p + 0.01)
    obs = torch.as_tensor(G["a_obs"][:, 0])
    plain.noise_in, ema.noise_in = Bank(G["a_noise"][:, :, :, -1]), Bank(G["a_noise"][:, :, :, -1])
    assert not torch.equal(plain.predict_batch(obs), ema.predict_batch(obs))


# ------------------------------------------------------------------------------------------------ the Philox stream
def test_rows_of_a_sub_batch_equal_the_rows_of_the_batch():
    obs = torch.as_tensor(G["a_obs"])
    whole, part = golden_policy("a", "cpu", seed=(7 << 32) | 5), golden_policy("a", "cpu", seed=(7 << 32) | 5)
    part.set_rollout_range(2, 3)
    whole.record = part.record = True
    for t in range(3):
        a, b = whole.predict_batch(obs[:, t]), part.predict_batch(obs[2:5, t])
        # the same draws bit for bit; the actions up to the f32 rounding of torch's layers on another batch shape (the replay bar; the kernel: bit for bit, on the GPU)
        assert torch.equal(whole.last_noise[:, 2:5], part.last_noise) and float((a[2:5] - b).abs().max()) <= 4 * float(G["a_D"])
        assert tuple(whole.last_noise.shape) == (5, 6, 2) and not whole.last_noise[4].any() and whole.last_noise[:4].abs().min() > 0
    other = golden_policy("a", "cpu", seed=(7 << 32) | 6)
    assert not torch.equal(other.predict_batch(obs[:, 0]), golden_policy("a", "cpu", seed=(7 << 32) | 5).predict_batch(obs[:, 0]))


def test_forks_advance_their_own_step_words():
    obs = torch.as_tensor(G["a_obs"])
    pol = golden_policy("a", "cpu", seed=3)
    pol.record = True
    first = pol.predict_batch(obs[:, 0]).clone()
    twin = pol.fork()
    assert twin.model is pol.model and twin._t is not pol._t and int(twin._t) == 1 and twin._packed is not pol._packed and twin.last_bad is None and twin.last_noise is None
    a, b = pol.predict_batch(obs[:, 1]), twin.predict_batch(obs[:, 1])
    assert torch.equal(a, b) and int(pol._t) == 2 and int(twin._t) == 2
    twin.predict_batch(obs[:, 2])
    assert int(pol._t) == 2 and int(twin._t) == 3
    again = golden_policy("a", "cpu", seed=3)
    assert torch.equal(again.predict_batch(obs[:, 0]), first) and not torch.equal(again.predict_batch(obs[:, 0]), first)      # same word, same draws; the next word, fresh ones


def test_normals_are_exact_on_the_philox_words():
    seed, off, n, t, k = (9 << 32) | 77, (1 << 33) + 5, 7, 0xFFFFFFF0, 3
    w = P.ddpm_mlp_words(seed, off, n, t, k)
    assert w.shape == (n, 2, 4) and w.dtype == np.uint32
    for row in (0, 6):
        for q in (0, 1):
            ge = off + row
            ref = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, P.DDPM_MLP_TAG | (k << 1) | q)
            assert [int(x) for x in ref] == w[row, q].tolist()
    z = P.ddpm_mlp_normals(seed, off, n, t, k, 8)
    assert z.shape == (n, 8) and z.dtype == np.float64 and np.array_equal(z, P.box_muller_f64(w).reshape(n, 8))
    assert np.array_equal(P.ddpm_mlp_normals(seed, off, n, t, k, 3), z[:, :3])
    assert not np.array_equal(P.ddpm_mlp_normals(seed, off, n, t, k + 1, 8), z)
    big = np.concatenate([P.ddpm_mlp_normals(1, 0, 4096, 0, k, 8).ravel() for k in range(4)])
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02


def test_the_tag_is_no_other_tags_upper_half():
    tags = {k: v for k, v in vars(P).items() if k.endswith("_TAG") and isinstance(v, int)}
    assert "DDPM_MLP_TAG" in tags and len(tags) >= 9
    assert all((v >> 16) != (P.DDPM_MLP_TAG >> 16) for k, v in tags.items() if k != "DDPM_MLP_TAG") and P.DDPM_MLP_TAG & 0xFFFF == 0 and P.DDPM_MLP_TAG >> 16
    assert capi.TAG_DDPM_MLP == P.DDPM_MLP_TAG
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "DDPM_MLP_TAG = 0x%08Xu" % P.DDPM_MLP_TAG in open(os.path.join(root, "d3il_amd", "csrc", "policy_ddpm_mlp.h")).read()
    assert (254 << 1 | 1) < (1 << 16) and P.DDPMNativePolicy.SWITCH == "D3IL_POLICY_DDPM_MLP_CHAIN"


# ------------------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("what", ["nan observation", "inf observation", "nan first draw", "nan step draw", "nan draw of the last step"])
def test_a_non_finite_lane_is_marked_and_no_other_lane_changes(what):
    obs = torch.as_tensor(G["a_obs"][:, 0]).clone()
    table = torch.as_tensor(G["a_noise"][:, :, :, -1]).clone()
    clean = golden_policy("a", "cpu", Bank(table.clone())).predict_batch(obs)
    if what.endswith("observation"):
        obs[3, 1] = float("nan") if what.startswith("nan") else float("inf")
    else:
        table[3, 0, {"nan first draw": 0, "nan step draw": 2, "nan draw of the last step": 4}[what], 1] = float("nan")
    pol = golden_policy("a", "cpu", Bank(table))
    y = pol.predict_batch(obs)
    if what == "nan draw of the last step":      # the reference's T + 1-th draw: never read
        assert torch.equal(y, clean) and pol.last_bad.tolist() == [0] * 6
        return
    others = [0, 1, 2, 4, 5]
    assert pol.last_bad.tolist() == [0, 0, 0, 1, 0, 0] and pol.last_bad.dtype == torch.int32
    assert bool(torch.isnan(y[3]).all()) and torch.equal(y[others], clean[others])


# ------------------------------------------------------------------------------------------------ packed tables
def test_packed_tables_follow_the_parameters():
    pol = golden_policy("a", "cpu")
    OBS, A, TD, T, W, HID, NHID = cfg("a")

    def tables():      # (PackedWeights refreshes its buffers in place: a snapshot)
        pol._packed.ensure(pol._pack_params(), pol._pack)
        return {k: v.clone() if torch.is_tensor(v) else v for k, v in pol._packed.buf.items()}

    w = tables()
    NT = HID // 16
    assert {"w_x", "w_state", "tbias", "temb", "w_blk", "b_blk", "w_out", "b_out", "sched", "bounds"} <= set(w)
    assert tuple(w["w_x"].shape) == (NT, 64, 2) and tuple(w["w_state"].shape) == (NT, 64, 16) and tuple(w["tbias"].shape) == (T, HID) and tuple(w["temb"].shape) == (T, TD)
    assert tuple(w["sched"].shape) == (T, 5) and float(w["sched"][0, 4]) == 0.0 and tuple(w["bounds"].shape) == (2 * A,)
    lin_in = pol.model.layers.layers[0]
    Wm = lin_in.weight.detach()
    # the packing: [T_out][lane (g, i)][s] = W[16 T_out + i][4 s + g] of the column group, zero beyond it
    for To, g, i, s in ((0, 0, 0, 0), (3, 1, 5, 0), (7, 3, 15, 0), (2, 2, 9, 1)):
        col = 4 * s + g
        assert float(w["w_x"][To, 16 * g + i, s]) == (float(Wm[16 * To + i, col]) if col < A else 0.0)
        assert float(w["w_state"][To, 16 * g + i, s]) == (float(Wm[16 * To + i, A + TD + col]) if col < OBS else 0.0)
    with torch.no_grad():
        temb = pol.model.temp_layers(torch.arange(T))
        assert torch.equal(w["temb"], temb) and torch.allclose(w["tbias"], temb @ Wm[:, A:A + TD].t() + lin_in.bias, atol=1e-6)
    assert torch.equal(w["sched"], P.ddpm_schedule(P.cosine_beta_schedule(T))["sched"])
    assert torch.equal(w["bounds"], torch.as_tensor(G["a_y_bounds"], dtype=torch.float32).reshape(-1))
    key = pol._packed.key
    pol.ensure_packed()      # (CPU: nothing to keep fresh for a kernel; the cache is untouched)
    assert pol._packed.key == key
    # load_state_dict and use_ema bump the version counters: the next ensure() repacks
    pol.load_reference_state_dict({k: v + 0.5 for k, v in golden_sd("a").items()})
    w2 = tables()
    assert not torch.equal(w2["tbias"], w["tbias"]) and float(w2["w_x"][0, 0, 0]) == float(Wm[0, 0]) != float(w["w_x"][0, 0, 0])
    pol.use_ema([p.detach().clone() * 0.5 for p in pol.model.parameters()])
    w3 = tables()
    assert torch.equal(w3["w_x"], 0.5 * w2["w_x"]) and not torch.equal(w3["temb"], w2["temb"])
    # param.data writes are invisible until invalidate_packed()
    pol.model.layers.layers[0].weight.data.mul_(2.0)
    assert torch.equal(tables()["w_x"], w3["w_x"])
    pol.invalidate_packed()
    assert torch.equal(tables()["w_x"], 2.0 * w3["w_x"])


def test_random_policy_has_the_sorting_four_shape_and_runs():
    pol = P.DDPMNativePolicy.random(16, 2, device="cpu", policy_seed=11)
    lin_in, blocks, lin_out = pol.model.layers._parts()
    assert (pol.obs_dim, pol.A, pol.t_dim, pol.T, lin_in.out_features, len(blocks), pol.seed) == (16, 2, 8, 4, 256, 4, 11) and pol._kernel_shape()
    y = pol.predict_batch(torch.zeros(5, 16))
    assert tuple(y.shape) == (5, 2) and y.dtype == torch.float32 and bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 0.002 * 1.5 + 1e-9
    small = P.DDPMNativePolicy.random(20, 3, device="cpu", hidden_dim=64, t_dim=8, n_timesteps=24)
    wide = P.DDPMNativePolicy.random(60, 2, device="cpu", hidden_dim=128, t_dim=4)
    assert not small._kernel_shape() and not wide._kernel_shape() and P.DDPMNativePolicy.random(58, 2, device="cpu", hidden_dim=128, t_dim=4)._kernel_shape()
