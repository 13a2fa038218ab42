"""policies.BESONativePolicy on the CPU against the reference's own BesoAgent + GCDenoiser + DiffusionGPT: tests/golden/ref_beso_agent.npz holds fixed-seed weights,
scaler statistics, observations, one banked normal per (environment, step, draw, position, component) and the reference's actions, rolled out batch-1 per environment
TWICE - in f32 as shipped and in f64 (tests/golden/gen_beso_goldens.py, run where the reference is).  D = max |f32 - f64| of the reference itself is the yardstick: the
replay has to stay within 4 D of the f64 table on every row (the chain is continuous in its inputs: no row is left out).  Draw 0 of a step is the init draw (it sits at
sequence index 0 of the bank and goes to position len - 1), draw 1 + i the noise of sampling step i, position by position; the last sampling step draws nothing.  The
gpu-marked replay of the same fixture is tests/test_gpu_policies_beso_native.py."""
import os
import types

import numpy as np
import torch

from d3il_amd import policies as P

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_beso_agent.npz"))
OBS, EMBD, LAYERS, HEADS, WINDOW, A, S = (int(v) for v in G["bs_cfg"])
SIGMA_MIN, SIGMA_MAX, SIGMA_DATA = (float(v) for v in G["bs_sigma"])
D = float(G["bs_D"])


def golden_sd():
    return {k[len("bs_sd__"):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith("bs_sd__")}


def golden_scaler(dev):
    return P.Scaler(G["bs_x_mean"], G["bs_x_std"], G["bs_y_mean"], G["bs_y_std"], G["bs_y_bounds"], device=dev)


def golden_policy(dev, noise_in=None, seed=0):
    net = P.DiffusionGPT(OBS, A, EMBD, LAYERS, HEADS, WINDOW)
    pol = P.BESONativePolicy(net.to(dev), golden_scaler(dev), WINDOW, S, SIGMA_MIN, SIGMA_MAX, sigma_data=SIGMA_DATA, seed=seed, noise_in=noise_in)
    pol.load_reference_state_dict(golden_sd())
    return pol


class Bank:
    """noise_in that replays table[:, call, d] ([n, calls, S, W, A]); a predict call starts with draw 0."""

    def __init__(self, table):
        self.table, self.call = torch.as_tensor(table, dtype=torch.float32), -1

    def __call__(self, d, n):
        if d == 0:
            self.call += 1
        return self.table[:n, self.call, d]


def replay(dev):
    """(worst |action - f64 table|, worst |action - f32 table|, policy) of the golden replay on ``dev``, all 48 rows."""
    pol = golden_policy(dev, Bank(G["bs_noise"]))
    obs = G["bs_obs"]
    w64 = w32 = 0.0
    for t in range(obs.shape[1]):
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        w64, w32 = max(w64, float(np.abs(a - G["bs_ref64"][:, t]).max())), max(w32, float(np.abs(a - G["bs_ref32"][:, t]).max()))
    return w64, w32, pol


def test_policy_rows_equal_reference_predict():
    assert float(np.abs(G["bs_ref32"] - G["bs_ref64"]).max()) == D and G["bs_ref64"].shape == (6, 8, A)
    w64, w32, pol = replay("cpu")
    print("golden replay (cpu): D %.3e, worst |action - f64 reference| %.3e (%.2f D), worst |action - f32 reference| %.3e" % (D, w64, w64 / D, w32))
    assert w64 <= 4 * D
    assert pol.hist.len.tolist() == [WINDOW] * 6 and int(pol._t) == 8 and pol.last_bad.tolist() == [0] * 6


def test_network_loads_the_reference_state_dict_and_hidden_is_the_forward():
    """load_reference_state_dict takes every parameter under ``inner_model.``, and hidden() on a hand-built token buffer gives what forward() computes."""
    net = P.DiffusionGPT(OBS, A, EMBD, LAYERS, HEADS, WINDOW)
    sd = {k[len("inner_model."):]: v for k, v in golden_sd().items() if k.startswith("inner_model.")}
    assert set(dict(net.named_parameters())) <= set(sd)
    net.load_state_dict({k: v for k, v in sd.items() if k in net.state_dict()})
    g = torch.Generator().manual_seed(2)
    states, x = torch.randn(3, WINDOW, OBS, generator=g) * 0.5, torch.randn(3, WINDOW, A, generator=g)
    with torch.no_grad():
        out = net(states, x, torch.full((3,), 0.3))
        xbuf = torch.empty(3, 2 * WINDOW + 1, EMBD)
        xbuf[:, 0] = net.sigma_emb(torch.tensor([[0.3]]).log() / 4)
        xbuf[:, 1::2] = net.tok_emb(states) + net.pos_emb[0, :WINDOW]
        xbuf[:, 2::2] = net.action_emb(x) + net.pos_emb[0, :WINDOW]
        out2 = net.action_pred(net.ln_f(net.hidden(xbuf, torch.arange(2, 2 * WINDOW + 1, 2))))
    assert tuple(out.shape) == (3, WINDOW, A) and float((out - out2).abs().max()) < 1e-5


def test_history_restart_of_single_lanes():
    """begin_episodes(mask): the restarted lane reproduces its first steps (same observations, same noise; its stale ring entries are never read) while the others go
    on with the reference's steps 3 .. 5."""
    n = 6
    noise, obs = torch.as_tensor(G["bs_noise"]), torch.as_tensor(G["bs_obs"])
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
        assert float(np.abs(again[t][2].numpy().astype(np.float64) - G["bs_ref64"][2, t]).max()) <= 4 * D
        assert float(np.abs(again[t][others].numpy().astype(np.float64) - G["bs_ref64"][others, 3 + t]).max()) <= 4 * D
    assert pol.hist.len.tolist() == [5, 5, 3, 5, 5, 5]


def test_ragged_batch_equals_per_lane_policies():
    """History lengths 1 .. 5 in ONE right-padded batch: every lane gets what a single-environment policy with the same history and the same noise computes (f32
    rounding of another batch shape: the replay bar)."""
    n, T = 5, 9
    gen = torch.Generator().manual_seed(21)
    obs = torch.randn(n, T, OBS, generator=gen) * 0.3
    noise = torch.randn(n, T, S, WINDOW, A, generator=gen)
    pol = golden_policy("cpu", Bank(noise))
    restarts = {4: [1], 5: [2], 6: [3], 7: [4]}      # before call 8 the lanes hold 5, 4, 3, 2, 1 observations
    out = []
    for t in range(T):
        if t in restarts:
            m = torch.zeros(n, dtype=torch.uint8); m[restarts[t]] = 1
            pol.begin_episodes(m)
        out.append(pol.predict_batch(obs[:, t]).clone())
        if t == 7:
            assert sorted(pol.hist.len.tolist()) == [1, 2, 3, 4, 5]
    assert pol.hist.len.tolist() == [5, 5, 4, 3, 2]
    for i in range(n):
        one = golden_policy("cpu", Bank(noise[i:i + 1]))
        for t in range(T):
            if t in restarts and i in restarts[t]:
                one.reset()
            a = one.predict_batch(obs[i:i + 1, t])
            np.testing.assert_allclose(a[0].numpy(), out[t][i].numpy(), atol=4 * D, err_msg="lane %d step %d" % (i, t))


def _stand_in_agent(use_ema=False, linear_output=True):
    """An object with the attributes from_reference reads off a live BesoAgent around GCDenoiser(DiffusionGPT), carrying the fixture's tensors."""
    net = P.DiffusionGPT(OBS, A, EMBD, LAYERS, HEADS, WINDOW, linear_output=linear_output)
    own = net.state_dict()
    net.load_state_dict({k[len("inner_model."):]: v for k, v in golden_sd().items() if k[len("inner_model."):] in own and (linear_output or "action_pred" not in k)}, strict=linear_output)
    net.goal_conditioned = False
    f64 = lambda k: torch.as_tensor(G[k], dtype=torch.float64)
    scaler = types.SimpleNamespace(x_mean=f64("bs_x_mean"), x_std=f64("bs_x_std"), y_mean=f64("bs_y_mean"), y_std=f64("bs_y_std"), y_bounds=G["bs_y_bounds"])
    shadow = [p.detach().clone() + 0.01 for p in net.parameters()]
    den = types.SimpleNamespace(inner_model=net, sigma_data=SIGMA_DATA, get_scalings=lambda sigma: None)
    return types.SimpleNamespace(model=den, scaler=scaler, window_size=WINDOW, use_ema=use_ema, gc=False, sampler_type="euler_ancestral", noise_scheduler="linear",
                                 num_sampling_steps=S, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX, sigma_data=SIGMA_DATA, action_context=[],
                                 ema_helper=types.SimpleNamespace(shadow_params=shadow), predict=lambda s: (_ for _ in ()).throw(AssertionError("the batched policy must not call predict")))


def test_from_reference_and_adapter_selection_and_fork():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = _stand_in_agent()
    assert P.BESONativePolicy.matches(agent) and not P.DDPMGPTPolicy.matches(agent) and not P.BeTPolicy.matches(agent)
    assert isinstance(as_batched(types.SimpleNamespace(predict=lambda s: s), 2), RowwiseAgent)
    # another sampler, another noise schedule or a goal-conditioned net keeps the agent on the row-by-row adapter (the reference's own code)
    for name, value in (("sampler_type", "euler"), ("sampler_type", "ddim"), ("noise_scheduler", "exponential"), ("noise_scheduler", "karras"), ("gc", True)):
        other = _stand_in_agent()
        setattr(other, name, value)
        other.predict = lambda s_: np.zeros((1, A))
        assert not P.BESONativePolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    goal = _stand_in_agent(); goal.model.inner_model.goal_conditioned = True
    goal.predict = lambda s_: np.zeros((1, A))
    assert not P.BESONativePolicy.matches(goal) and isinstance(as_batched(goal, 2), RowwiseAgent)
    # the Linear-SiLU-Linear head is accepted and runs the torch glue
    mlp = _stand_in_agent(linear_output=False)
    assert P.BESONativePolicy.matches(mlp)
    mp = as_batched(mlp, 2)
    assert isinstance(mp, P.BESONativePolicy) and not mp.step_kernel_ok(torch.device("cuda:0")) and isinstance(mp.model.action_pred, torch.nn.Sequential)
    assert tuple(mp.predict_batch(torch.as_tensor(G["bs_obs"][:2, 0])).shape) == (2, A)
    pol = as_batched(agent, 6)
    assert isinstance(pol, P.BESONativePolicy) and pol.S == S and pol.W == WINDOW and pol.model is not agent.model.inner_model
    assert (pol.sigma_min, pol.sigma_max, pol.sigma_data) == (SIGMA_MIN, SIGMA_MAX, SIGMA_DATA)
    pol.noise_in = Bank(G["bs_noise"])
    for t in range(3):
        a = pol.predict_batch(torch.as_tensor(G["bs_obs"][:, t]))
        assert float(np.abs(a.numpy().astype(np.float64) - G["bs_ref64"][:, t]).max()) <= 4 * D
    twin = pol.fork()
    assert twin.model is pol.model and twin.hist is None and twin.a_hist is None and twin._t is not pol._t and int(twin._t) == 3 and twin._packed is not pol._packed
    twin.noise_in = Bank(G["bs_noise"])
    twin.predict_batch(torch.as_tensor(G["bs_obs"][:, 0]))
    assert pol.hist.len.tolist() == [3] * 6 and twin.hist.len.tolist() == [1] * 6 and int(pol._t) == 3 and int(twin._t) == 4
    assert twin.a_hist is not pol.a_hist
    # use_ema: the shadow parameters are what the policy runs on, and the packed tables follow them
    ema = P.BESONativePolicy.from_reference(_stand_in_agent(use_ema=True))
    for p, q in zip(ema.model.parameters(), agent.model.inner_model.parameters()):
        assert torch.equal(p, q + 0.01)
    ema.ensure_packed()
    before = ema._packed.buf["bias_pos"].clone()
    ema.use_ema([p.detach() for p in agent.model.inner_model.parameters()])
    ema.ensure_packed()
    assert float((ema._packed.buf["bias_pos"] - (before - 0.02)).abs().max()) < 1e-6


OTHER_TAGS = {"BET_TAG": 0x42655448, "DDPM_GPT_TAG": 0x44470000, "IBC_TAG": 0x49420000, "ACT_TAG": 0x41430000, "CVAE_TAG": 0x43560000, "DDPM_ACT_TAG": 0x44410000,
              "BET_MLP_TAG": 0x424D4C50}


def test_host_normals():
    """beso_normals: the words are Philox4x32-10 of the stated counters, the normals Box-Muller of them; moments over 2^20 normals; every counter field matters; the tag
    shares no word with the other policies' layouts; a rollout range is a slice of the whole."""
    from d3il_amd import capi
    seed, off, t, d, W = 0x1234567890ABCDEF, (1 << 32) - 3, 7, 5, 5
    w = P.beso_words(seed, off, 6, t, d, W)
    assert w.shape == (6, W, 2, 4) and w.dtype == np.uint32
    for n in range(6):
        ge = off + n
        for j in range(W):
            for q in range(2):
                want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x42530000 | d << 8 | j << 1 | q)
                assert [int(x) for x in want] == w[n, j, q].tolist()
    z = P.beso_normals(seed, off, 6, t, d, W, 8)
    r = w[1, 3, 1].astype(np.float64)
    u1, u2 = (np.floor(r[2] / 256) + 1) / 2 ** 24, np.floor(r[3] / 256) / 2 ** 24
    assert z[1, 3, 6] == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2) and z[1, 3, 7] == np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)
    assert np.array_equal(P.beso_normals(seed, off, 6, t, d, W, 3), z[:, :, :3])
    big = P.beso_normals(3, 0, 8192, 0, 8, 16, 8)
    n = big.size
    assert n >= 1 << 20 and np.isfinite(big).all()
    print("moments over %d normals: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e)" % (n, big.mean(), 5 / np.sqrt(n), big.var() - 1, 5 * np.sqrt(2 / n)))
    assert abs(big.mean()) < 5 / np.sqrt(n) and abs(big.var() - 1) < 5 * np.sqrt(2 / n)
    # every counter field changes the words: seed, rollout offset, step word, draw index, position, q
    base = P.beso_words(seed, 0, 4, t, d, W)
    for other in (P.beso_words(seed + 1, 0, 4, t, d, W), P.beso_words(seed ^ (1 << 40), 0, 4, t, d, W), P.beso_words(seed, 1, 4, t, d, W), P.beso_words(seed, 1 << 32, 4, t, d, W),
                  P.beso_words(seed, 0, 4, t + 1, d, W), P.beso_words(seed, 0, 4, t, d + 1, W), P.beso_words(seed, 0, 4, t, 0, W)):
        assert not np.array_equal(base, other) and not (base == other).all(axis=-1).any()
    assert np.array_equal(P.beso_words(seed, 1, 3, t, d, W), P.beso_words(seed, 0, 4, t, d, W)[1:])
    assert len({tuple(base[0, j, q]) for j in range(W) for q in range(2)}) == 2 * W
    assert len({tuple(x) for x in np.concatenate([P.beso_words(seed, 0, 4, tt, dd, W).reshape(-1, 4) for tt in (0, 1) for dd in (0, 1, 15)])}) == 6 * 4 * W * 2
    # the tag: BESO words are 0x4253 in the upper half (draw <= 254, j <= 15, q <= 1 stay below bit 16); no other tag has that upper half, and 0 is the harness's
    assert P.BESO_TAG == capi.BESO_TAG == 0x42530000 and (254 << 8 | 15 << 1 | 1) < 1 << 16
    for name, tag in OTHER_TAGS.items():
        assert getattr(capi, name) == tag and tag >> 16 != P.BESO_TAG >> 16, name
    assert sorted(k for k in vars(capi) if k.endswith("_TAG")) == sorted(list(OTHER_TAGS) + ["BESO_TAG"])
    # the policy's default draw: a rollout range is the matching slice of the whole batch
    obs = torch.as_tensor(G["bs_obs"])
    whole, part = golden_policy("cpu", seed=5), golden_policy("cpu", seed=5)
    whole.record = part.record = True
    part.set_rollout_range(2, 3)
    for s in range(2):
        a, b = whole.predict_batch(obs[:, s]), part.predict_batch(obs[2:5, s])
        assert sorted(whole.last_noise) == list(range(S + 1))
        for dd in range(S):
            assert torch.equal(whole.last_noise[dd][2:5], part.last_noise[dd])
            want = P.beso_normals(5, 0, 6, s, dd, WINDOW, A).astype(np.float32)
            if dd == 0:
                want[:, 1:] = 0      # the init draw: one per environment, recorded at j = 0
            assert np.array_equal(whole.last_noise[dd].numpy(), want)
        assert not whole.last_noise[S].any()      # the last sampling step draws nothing
        assert float((a[2:5] - b).abs().max()) <= 4 * D      # (torch's CPU GEMM rounds a 3-row and a 6-row batch differently; the draw itself is identical)


def test_packed_tables():
    """semb = sigma_emb(log(sigma) / 4) of the f32 linear schedule, bias_pos = action_emb.bias + pos_emb[:W], coef = the reference's scalings and ancestral steps."""
    pol = golden_policy("cpu")
    pol.ensure_packed()
    w, m = pol._packed.buf, pol.model
    sig = torch.cat([torch.linspace(SIGMA_MAX, SIGMA_MIN, S), torch.zeros(1)])
    assert pol.sigmas == sig.tolist() == P.BESOPolicy(m, golden_scaler("cpu"), WINDOW, S, SIGMA_MIN, SIGMA_MAX).sigmas
    s64 = sig.double()
    sd2 = SIGMA_DATA ** 2
    want = torch.zeros(S, 6, dtype=torch.float64)
    for i in range(S):
        s_from, s_to = s64[i], s64[i + 1]
        s_up = min(s_to, (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5)      # gc_sampling.get_ancestral_step, eta = 1
        s_down = (s_to ** 2 - s_up ** 2) ** 0.5
        want[i] = torch.stack([sd2 / (s_from ** 2 + sd2), s_from * SIGMA_DATA / (s_from ** 2 + sd2) ** 0.5, 1 / s_from, s_down - s_from, s_up,
                               1 / (s_to ** 2 + sd2) ** 0.5 if i < S - 1 else torch.zeros((), dtype=torch.float64)])
    assert tuple(w["coef"].shape) == (S, 6) and w["coef"].dtype == torch.float32 and torch.equal(w["coef"], want.float())
    assert float(w["coef"][S - 1, 4]) == 0.0 and bool((w["coef"][:S - 1, 4] > 0).all()) and float(w["coef"][S - 1, 3]) == -float(sig[S - 1])
    assert pol.c_in0 == float(1 / (s64[0] ** 2 + sd2) ** 0.5)
    with torch.no_grad():
        assert torch.equal(w["semb"], m.sigma_emb(sig[:S].reshape(-1, 1).log() / 4)) and tuple(w["semb"].shape) == (S, EMBD)
        assert torch.equal(w["bias_pos"], m.action_emb.bias + m.pos_emb[0, :WINDOW]) and tuple(w["bias_pos"].shape) == (WINDOW, EMBD)


def test_nonfinite_hidden_row_marks_its_lane_only():
    pol = golden_policy("cpu", Bank(G["bs_noise"]))
    obs = torch.as_tensor(G["bs_obs"][:, 0]).clone()
    clean = pol.predict_batch(obs).clone()
    pol.noise_in.call = -1
    pol.reset()
    obs[3, 4] = float("nan")
    y = pol.predict_batch(obs)
    assert pol.last_bad.tolist() == [0, 0, 0, 1, 0, 0] and bool(torch.isnan(y[3]).all()) and bool(torch.isnan(pol.a_hist[3, -1]).all())
    assert torch.equal(y[[0, 1, 2, 4, 5]], clean[[0, 1, 2, 4, 5]])


def test_range_guard_interface_and_refusals():
    """What simulation/_rollout.py duck-types on, and the constructor's limits."""
    import pytest
    pol = golden_policy("cpu")
    assert hasattr(pol, "weights_out_of_range") and hasattr(pol, "range_report") and pol.f16x3_blocks is False      # (a 32-wide net: no split-f16 blocks)
    with pytest.raises(RuntimeError, match="no RangeGuard is enabled"):
        pol.range_report()
    with pytest.raises(AssertionError):
        P.BESONativePolicy(P.DiffusionGPT(OBS, A, EMBD, LAYERS, HEADS, WINDOW), golden_scaler("cpu"), WINDOW, 255, SIGMA_MIN, SIGMA_MAX)
    with pytest.raises(AssertionError):
        P.BESONativePolicy(P.DiffusionGPT(OBS, A, EMBD, LAYERS, HEADS, WINDOW), golden_scaler("cpu"), WINDOW + 1, S, SIGMA_MIN, SIGMA_MAX)
    assert P.BESONativePolicy.SWITCH == "D3IL_POLICY_BESO_STEP"
