"""policies.DDPMGPTPolicy on the CPU against the reference's own DiffusionAgent + Diffusion + DiffusionTransformerNetwork: tests/golden/ref_ddpm_gpt_agent.npz holds
fixed-seed weights, scaler statistics, observations, one banked normal per (environment, step, chain index, position, component) and the reference's actions, rolled out
batch-1 per environment TWICE - in f32 as shipped and in f64 (tests/golden/gen_ddpm_gpt_goldens.py, run where the reference is).  D = max |f32 - f64| of the reference
itself is the yardstick: the replay has to stay within 4 D of the f64 table on every row (the chain is continuous in its inputs: no row is left out).  The gpu-marked
replay of the same fixture is tests/test_gpu_policies_ddpm_gpt.py."""
import os
import types

import numpy as np
import torch

from d3il_amd import policies as P

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ddpm_gpt_agent.npz"))
OBS, EMBD, LAYERS, HEADS, WINDOW, A, T = (int(v) for v in G["dg_cfg"])
D = float(G["dg_D"])


def golden_sd():
    return {k[len("dg_sd__"):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith("dg_sd__")}


def golden_scaler(dev):
    return P.Scaler(G["dg_x_mean"], G["dg_x_std"], G["dg_y_mean"], G["dg_y_std"], G["dg_y_bounds"], device=dev)


def golden_policy(dev, noise_in=None, seed=0):
    den = P.DiffusionGPTDenoiser(OBS, A, EMBD, LAYERS, HEADS, WINDOW)
    pol = P.DDPMGPTPolicy(den.to(dev), golden_scaler(dev), T, WINDOW, seed=seed, noise_in=noise_in)
    pol.load_reference_state_dict(golden_sd())
    return pol


class Bank:
    """noise_in that replays table[:, call, k] ([n, calls, T + 1, W, A]); a predict call starts with chain index T."""

    def __init__(self, table):
        self.table, self.call = torch.as_tensor(table, dtype=torch.float32), -1

    def __call__(self, k, n):
        if k == T:
            self.call += 1
        return self.table[:n, self.call, k]


def replay(dev):
    """(worst |action - f64 table|, worst |action - f32 table|, policy) of the golden replay on ``dev``, all 48 rows."""
    pol = golden_policy(dev, Bank(G["dg_noise"]))
    obs = G["dg_obs"]
    w64 = w32 = 0.0
    for t in range(obs.shape[1]):
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        w64, w32 = max(w64, float(np.abs(a - G["dg_ref64"][:, t]).max())), max(w32, float(np.abs(a - G["dg_ref32"][:, t]).max()))
    return w64, w32, pol


def test_policy_rows_equal_reference_predict():
    assert float(np.abs(G["dg_ref32"] - G["dg_ref64"]).max()) == D and G["dg_ref64"].shape == (6, 8, A)
    w64, w32, pol = replay("cpu")
    print("golden replay (cpu): D %.3e, worst |action - f64 reference| %.3e (%.2f D), worst |action - f32 reference| %.3e" % (D, w64, w64 / D, w32))
    assert w64 <= 4 * D
    assert pol.hist.len.tolist() == [WINDOW] * 6 and int(pol._t) == 8 and pol.last_bad.tolist() == [0] * 6


def test_denoiser_loads_the_reference_state_dict_and_forward_is_the_chain_step():
    """load_state_dict takes every entry under ``model.`` (no missing, no unexpected key), and forward() - the reference's signature - gives the eps the sampler's
    token-buffer form computes."""
    den = P.DiffusionGPTDenoiser(OBS, A, EMBD, LAYERS, HEADS, WINDOW)
    res = den.load_state_dict({k[len("model."):]: v for k, v in golden_sd().items() if k.startswith("model.")})
    assert not res.missing_keys and not res.unexpected_keys
    assert all(k.startswith("model.") for k in golden_sd())
    g = torch.Generator().manual_seed(2)
    states, x = torch.randn(3, WINDOW, OBS, generator=g) * 0.5, torch.randn(3, WINDOW, A, generator=g)
    with torch.no_grad():
        eps = den(x, torch.full((3,), 5), states)
        xbuf = torch.empty(3, 2 * WINDOW + 1, EMBD)
        xbuf[:, 0] = den.time_emb(torch.tensor([5]))
        xbuf[:, 1::2] = den.tok_emb(states) + den.pos_emb[0, :WINDOW]
        xbuf[:, 2::2] = den.action_emb(x) + den.pos_emb[0, :WINDOW]
        eps2 = den.action_pred(den.ln_f(den.hidden(xbuf, torch.arange(2, 2 * WINDOW + 1, 2))))
    assert tuple(eps.shape) == (3, WINDOW, A) and float((eps - eps2).abs().max()) < 1e-5
    gelu = P.DiffusionGPTDenoiser(OBS, A, EMBD, LAYERS, HEADS, WINDOW, linear_output=False)
    assert sorted(k for k in gelu.state_dict() if k.startswith("action_pred")) == ["action_pred.0.bias", "action_pred.0.weight", "action_pred.2.bias", "action_pred.2.weight"]


def test_history_restart_of_single_lanes():
    """begin_episodes(mask): the restarted lane reproduces its first steps (same observations, same noise) while the others go on with the reference's steps 3 .. 5."""
    n = 6
    noise, obs = torch.as_tensor(G["dg_noise"]), torch.as_tensor(G["dg_obs"])
    mask = torch.zeros(n, dtype=torch.uint8); mask[2] = 1
    m5 = mask.bool().view(n, 1, 1, 1, 1)
    table = torch.cat((noise[:, :3], torch.where(m5, noise[:, :3], noise[:, 3:6])), dim=1)
    pol = golden_policy("cpu", Bank(table))
    first = [pol.predict_batch(obs[:, t]).clone() for t in range(3)]
    pol.begin_episodes(mask)
    again = [pol.predict_batch(torch.where(mask.bool().unsqueeze(1), obs[:, t], obs[:, 3 + t])).clone() for t in range(3)]
    others = [i for i in range(n) if i != 2]
    for t in range(3):
        np.testing.assert_allclose(again[t][2].numpy(), first[t][2].numpy(), atol=4 * D)
        assert float(np.abs(again[t][2].numpy().astype(np.float64) - G["dg_ref64"][2, t]).max()) <= 4 * D
        assert float(np.abs(again[t][others].numpy().astype(np.float64) - G["dg_ref64"][others, 3 + t]).max()) <= 4 * D
    assert pol.hist.len.tolist() == [5, 5, 3, 5, 5, 5]


def test_ragged_batch_equals_per_lane_policies():
    """History lengths 1 .. 5 in ONE right-padded batch: every lane gets what a single-environment policy with the same history and the same noise computes (f32
    rounding of another batch shape: the replay bar)."""
    n, S = 5, 9
    gen = torch.Generator().manual_seed(21)
    obs = torch.randn(n, S, OBS, generator=gen) * 0.3
    noise = torch.randn(n, S, T + 1, WINDOW, A, generator=gen)
    pol = golden_policy("cpu", Bank(noise))
    restarts = {4: [1], 5: [2], 6: [3], 7: [4]}      # before call 8 the lanes hold 5, 4, 3, 2, 1 observations
    out = []
    for t in range(S):
        if t in restarts:
            m = torch.zeros(n, dtype=torch.uint8); m[restarts[t]] = 1
            pol.begin_episodes(m)
        out.append(pol.predict_batch(obs[:, t]).clone())
        if t == 7:
            assert sorted(pol.hist.len.tolist()) == [1, 2, 3, 4, 5]
    assert pol.hist.len.tolist() == [5, 5, 4, 3, 2]
    for i in range(n):
        one = golden_policy("cpu", Bank(noise[i:i + 1]))
        for t in range(S):
            if t in restarts and i in restarts[t]:
                one.reset()
            a = one.predict_batch(obs[i:i + 1, t])
            np.testing.assert_allclose(a[0].numpy(), out[t][i].numpy(), atol=4 * D, err_msg="lane %d step %d" % (i, t))


def _stand_in_agent(use_ema=False):
    """An object with the attributes from_reference reads off a live DiffusionAgent around a DiffusionTransformerNetwork, carrying the fixture's tensors."""
    net = P.DiffusionGPTDenoiser(OBS, A, EMBD, LAYERS, HEADS, WINDOW)
    net.load_state_dict({k[len("model."):]: v for k, v in golden_sd().items()})
    f64 = lambda k: torch.as_tensor(G[k], dtype=torch.float64)
    scaler = types.SimpleNamespace(x_mean=f64("dg_x_mean"), x_std=f64("dg_x_std"), y_mean=f64("dg_y_mean"), y_std=f64("dg_y_std"), y_bounds=G["dg_y_bounds"])
    shadow = [p.detach().clone() + 0.01 for p in net.parameters()]
    diff = types.SimpleNamespace(model=net, n_timesteps=T, betas=P.cosine_beta_schedule(T), predict_epsilon=True, clip_denoised=True, diffusion_x=False)
    return types.SimpleNamespace(model=diff, scaler=scaler, window_size=WINDOW, use_ema=use_ema, diffusion_kde=False,
                                 ema_helper=types.SimpleNamespace(shadow_params=shadow), predict=lambda s: (_ for _ in ()).throw(AssertionError("the batched policy must not call predict")))


def test_from_reference_and_adapter_selection_and_fork():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = _stand_in_agent()
    assert P.DDPMGPTPolicy.matches(agent) and not P.BeTPolicy.matches(agent)
    # a DDPM-MLP agent (DiffusionMLPNetwork: no time_emb / action_emb / blocks) keeps going row by row, as does anything else
    mlp_agent = types.SimpleNamespace(model=types.SimpleNamespace(model=P.DiffusionMLP(2, 16, 8, 32, 4), n_timesteps=4), scaler=agent.scaler, window_size=1, predict=lambda s: s)
    assert not P.DDPMGPTPolicy.matches(mlp_agent) and isinstance(as_batched(mlp_agent, 2), RowwiseAgent)
    assert isinstance(as_batched(types.SimpleNamespace(predict=lambda s: s), 2), RowwiseAgent)
    goal = _stand_in_agent(); goal.model.model.goal_conditioned = True
    assert not P.DDPMGPTPolicy.matches(goal)
    # every switch of the reference's configuration that selects another sampler keeps the agent on the row-by-row adapter (the reference's own code)
    for where, name, value in (("model", "diffusion_x", True), ("model", "predict_epsilon", False), ("model", "clip_denoised", False), ("agent", "diffusion_kde", True),
                               ("model", "betas", torch.linspace(1e-4, 2e-2, T)), ("model", "betas", P.cosine_beta_schedule(T + 1))):
        other = _stand_in_agent()
        setattr(other.model if where == "model" else other, name, value)
        other.predict = lambda s_: np.zeros((1, A))
        assert not P.DDPMGPTPolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    no_betas = _stand_in_agent(); del no_betas.model.betas
    assert not P.DDPMGPTPolicy.matches(no_betas)
    pol = as_batched(agent, 6)
    assert isinstance(pol, P.DDPMGPTPolicy) and pol.T == T and pol.W == WINDOW and pol.model is not agent.model.model
    pol.noise_in = Bank(G["dg_noise"])
    for t in range(3):
        a = pol.predict_batch(torch.as_tensor(G["dg_obs"][:, t]))
        assert float(np.abs(a.numpy().astype(np.float64) - G["dg_ref64"][:, t]).max()) <= 4 * D
    twin = pol.fork()
    assert twin.model is pol.model and twin.hist is None and twin._t is not pol._t and int(twin._t) == 3 and twin._packed is not pol._packed
    twin.noise_in = Bank(G["dg_noise"])
    twin.predict_batch(torch.as_tensor(G["dg_obs"][:, 0]))
    assert pol.hist.len.tolist() == [3] * 6 and twin.hist.len.tolist() == [1] * 6 and int(pol._t) == 3 and int(twin._t) == 4
    # use_ema: the shadow parameters are what the policy runs on, and the packed tables follow them
    ema = P.DDPMGPTPolicy.from_reference(_stand_in_agent(use_ema=True))
    for p, q in zip(ema.model.parameters(), agent.model.model.parameters()):
        assert torch.equal(p, q + 0.01)
    ema.ensure_packed()
    before = ema._packed.buf["bias_pos"].clone()
    ema.use_ema([p.detach() for p in agent.model.model.parameters()])
    ema.ensure_packed()
    assert float((ema._packed.buf["bias_pos"] - (before - 0.02)).abs().max()) < 1e-6


def test_host_normals():
    """ddpm_gpt_normals: the words are Philox4x32-10 of the stated counters, the normals Box-Muller of them; moments over 2^20 normals; every counter field matters; a
    rollout range is a slice of the whole."""
    seed, off, t, k, W = 0x1234567890ABCDEF, (1 << 32) - 3, 7, 5, 5
    w = P.ddpm_gpt_words(seed, off, 6, t, k, W)
    assert w.shape == (6, W, 2, 4) and w.dtype == np.uint32
    for n in range(6):
        ge = off + n
        for j in range(W):
            for q in range(2):
                want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x44470000 | k << 8 | j << 1 | q)
                assert [int(x) for x in want] == w[n, j, q].tolist()
    z = P.ddpm_gpt_normals(seed, off, 6, t, k, W, 8)
    r = w[1, 3, 1].astype(np.float64)
    u1, u2 = (np.floor(r[2] / 256) + 1) / 2 ** 24, np.floor(r[3] / 256) / 2 ** 24
    assert z[1, 3, 6] == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2) and z[1, 3, 7] == np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)
    assert np.array_equal(P.ddpm_gpt_normals(seed, off, 6, t, k, W, 3), z[:, :, :3])
    big = P.ddpm_gpt_normals(3, 0, 8192, 0, 8, 16, 8)
    n = big.size
    assert n >= 1 << 20 and np.isfinite(big).all()
    print("moments over %d normals: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e)" % (n, big.mean(), 5 / np.sqrt(n), big.var() - 1, 5 * np.sqrt(2 / n)))
    assert abs(big.mean()) < 5 / np.sqrt(n) and abs(big.var() - 1) < 5 * np.sqrt(2 / n)
    base = P.ddpm_gpt_words(seed, 0, 4, t, k, W)
    assert not np.array_equal(base, P.ddpm_gpt_words(seed, 0, 4, t, k + 1, W)) and not np.array_equal(base, P.ddpm_gpt_words(seed, 0, 4, t + 1, k, W))
    assert len({tuple(base[0, j, q]) for j in range(W) for q in range(2)}) == 2 * W
    assert len({tuple(x) for x in np.concatenate([P.ddpm_gpt_words(seed, 0, 4, tt, kk, W).reshape(-1, 4) for tt in (0, 1) for kk in (1, 2, 8)])}) == 6 * 4 * W * 2
    # the policy's default draw: a rollout range is the matching slice of the whole batch
    obs = torch.as_tensor(G["dg_obs"])
    whole, part = golden_policy("cpu", seed=5), golden_policy("cpu", seed=5)
    whole.record = part.record = True
    part.set_rollout_range(2, 3)
    for s in range(2):
        a, b = whole.predict_batch(obs[:, s]), part.predict_batch(obs[2:5, s])
        for kk in range(1, T + 1):
            assert torch.equal(whole.last_noise[kk][2:5], part.last_noise[kk])
            assert np.array_equal(whole.last_noise[kk].numpy(), P.ddpm_gpt_normals(5, 0, 6, s, kk, WINDOW, A).astype(np.float32))
        assert float((a[2:5] - b).abs().max()) <= 4 * D      # (torch's CPU GEMM rounds a 3-row and a 6-row batch differently; the draw itself is identical)


def test_packed_tables():
    """temb = time_emb(arange(T)), bias_pos = action_emb.bias + pos_emb[:W], and the schedule table is DDPMPolicy's for the same T (policies.ddpm_schedule)."""
    pol = golden_policy("cpu")
    pol.ensure_packed()
    w, m = pol._packed.buf, pol.model
    mlp = P.DDPMPolicy(P.DiffusionMLP(A, OBS, 8, 32, 4), golden_scaler("cpu"), T)
    sig = (0.5 * mlp.post_logvar).exp() * torch.cat((torch.zeros(1), torch.ones(T - 1)))
    sched = torch.stack((mlp.sqrt_recip_ac, mlp.sqrt_recipm1_ac, mlp.coef1, mlp.coef2, sig), dim=1)
    assert tuple(w["sched"].shape) == (T, 5) and torch.equal(w["sched"], sched) and float(w["sched"][0, 4]) == 0.0 and bool((w["sched"][1:, 4] > 0).all())
    assert torch.equal(w["sched"], P.ddpm_schedule(P.cosine_beta_schedule(T))["sched"]) and torch.equal(mlp._sched, w["sched"])      # one helper behind both policies
    s64 = P.ddpm_schedule(P.cosine_beta_schedule(T).double())["sched"]
    assert s64.dtype == torch.float64 and float((s64 - w["sched"].double()).abs().max() / s64.abs().max()) < 1e-6
    with torch.no_grad():
        assert torch.equal(w["temb"], m.time_emb(torch.arange(T))) and tuple(w["temb"].shape) == (T, EMBD)
        assert torch.equal(w["bias_pos"], m.action_emb.bias + m.pos_emb[0, :WINDOW]) and tuple(w["bias_pos"].shape) == (WINDOW, EMBD)


def test_nonfinite_hidden_row_marks_its_lane_only():
    pol = golden_policy("cpu", Bank(G["dg_noise"]))
    obs = torch.as_tensor(G["dg_obs"][:, 0]).clone()
    clean = pol.predict_batch(obs).clone()
    pol.noise_in.call = -1
    pol.reset()
    obs[3, 4] = float("nan")
    y = pol.predict_batch(obs)
    assert pol.last_bad.tolist() == [0, 0, 0, 1, 0, 0] and bool(torch.isnan(y[3]).all())
    assert torch.equal(y[[0, 1, 2, 4, 5]], clean[[0, 1, 2, 4, 5]])
