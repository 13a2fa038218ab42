"""policies.BeTPolicy on the CPU against the reference's own BeT_Agent: tests/golden/ref_bet_agent.npz holds fixed-seed weights, scaler statistics, bin centres,
observations, one banked uniform per (environment, step) and the reference's bins, actions and last-token logits, rolled out batch-1 per environment
(tests/golden/gen_bet_goldens.py, run where the reference is; no banked u lies within 1e-4 of an edge of its row's CDF, so no row is left out).  The gpu-marked
replay of the same fixture is tests/test_gpu_policies_bet.py."""
import os
import types

import numpy as np
import torch

from d3il_amd import policies as P

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_bet_agent.npz"))
OBS, EMBD, LAYERS, HEADS, WINDOW, V, A = (int(v) for v in G["bet_cfg"])
BAR = 5e-6      # the bar of test_policies.test_beso_policy_rows_equal_reference_predict (same block type through 16 forwards): one forward gets the same bar


def golden_sd():
    return {k[len("bet_sd__"):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith("bet_sd__")}


def golden_scaler(dev):
    return P.Scaler(G["bet_x_mean"], G["bet_x_std"], G["bet_y_mean"], G["bet_y_std"], G["bet_y_bounds"], device=dev)


def golden_policy(dev, uniform_fn=None, seed=0):
    trunk = P.MinGPTTrunk(OBS, EMBD, LAYERS, HEADS, WINDOW, V, A)
    trunk.load_state_dict(golden_sd())
    sc = golden_scaler(dev)
    return P.BeTPolicy(trunk.to(dev), G["bet_centers"], sc, sc.y_bounds[0], sc.y_bounds[1], WINDOW, seed=seed, uniform_fn=uniform_fn)


class Bank:
    """uniform_fn that replays column t of a [n, T] table at call t."""

    def __init__(self, table):
        self.table, self.call = torch.as_tensor(table, dtype=torch.float32), 0

    def __call__(self, n):
        self.call += 1
        return self.table[:n, self.call - 1]


def replay(dev):
    """(bins equal everywhere?, worst |action - reference|, worst |last-token logit - reference|) of the golden replay on ``dev``; on a HIP device the logits are
    compared as log-probabilities (the head kernel returns probabilities)."""
    pol = golden_policy(dev, Bank(G["bet_u"]))
    pol.record = True
    obs, ref, bins, logits = G["bet_obs"], G["bet_ref"], G["bet_bins"], torch.as_tensor(G["bet_logits"])
    same, worst_a, worst_l = True, 0.0, 0.0
    for t in range(obs.shape[1]):
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev))
        same = same and np.array_equal(pol.last_bins.cpu().numpy().astype(np.int64), bins[:, t])
        worst_a = max(worst_a, float(np.abs(a.cpu().numpy().astype(np.float64) - ref[:, t]).max()))
        if pol.last_logits is not None:
            worst_l = max(worst_l, float((pol.last_logits.cpu() - logits[:, t]).abs().max()))
        else:
            worst_l = max(worst_l, float((pol.last_probs.cpu().log() - torch.log_softmax(logits[:, t], dim=1)).abs().max()))
    return same, worst_a, worst_l, pol


def test_bet_policy_rows_equal_reference_predict():
    same, worst_a, worst_l, pol = replay("cpu")
    print("golden replay (cpu): worst |action - reference| %.3e, worst |logit - reference| %.3e" % (worst_a, worst_l))
    assert same                                  # every environment, every step: no row left out
    assert worst_a < BAR and worst_l < BAR
    assert pol.hist.len.tolist() == [WINDOW] * G["bet_obs"].shape[0] and int(pol._t) == G["bet_obs"].shape[1]


def test_trunk_loads_the_reference_state_dict_and_equals_the_full_forward():
    """MinGPTTrunk.forward (every position, ln_f, head) is the reference GPT's forward: the last-token logits of a full window equal the golden ones, and
    hidden(keep=[last]) is the last row of hidden()."""
    trunk = P.MinGPTTrunk(OBS, EMBD, LAYERS, HEADS, WINDOW, V, A)
    missing = trunk.load_state_dict(golden_sd())
    assert not missing.missing_keys and not missing.unexpected_keys
    sc = golden_scaler("cpu")
    x = sc.scale_input(torch.as_tensor(G["bet_obs"][:, :WINDOW], dtype=torch.float32))
    with torch.no_grad():
        out = trunk(x)
        h_all, h_last = trunk.hidden(x), trunk.hidden(x, keep=torch.tensor([WINDOW - 1]))
    assert tuple(out.shape) == (x.shape[0], WINDOW, V * (1 + A))
    assert float((out[:, -1, :V] - torch.as_tensor(G["bet_logits"][:, WINDOW - 1])).abs().max()) < BAR
    assert float((h_all[:, -1:] - h_last).abs().max()) < 1e-6


def test_history_restart_of_single_lanes():
    """begin_episodes(mask): the restarted lane reproduces its first steps (same observations, same u) while the others keep their windows."""
    n = G["bet_obs"].shape[0]
    u = torch.as_tensor(G["bet_u"])
    obs = torch.as_tensor(G["bet_obs"])
    mask = torch.zeros(n, dtype=torch.uint8); mask[2] = 1
    table = torch.cat((u[:, :3], torch.where(mask.bool().unsqueeze(1), u[:, :3], u[:, 3:6])), dim=1)
    pol = golden_policy("cpu", Bank(table))
    first = [(pol.predict_batch(obs[:, t]).clone(), pol.last_bins.clone()) for t in range(3)]
    pol.begin_episodes(mask)
    again = [(pol.predict_batch(torch.where(mask.bool().unsqueeze(1), obs[:, t], obs[:, 3 + t])).clone(), pol.last_bins.clone()) for t in range(3)]
    for t in range(3):
        assert int(again[t][1][2]) == int(first[t][1][2]) == int(G["bet_bins"][2, t])
        np.testing.assert_allclose(again[t][0][2].numpy(), first[t][0][2].numpy(), atol=1e-6)
        # the lanes that went on: the reference's steps 3 .. 5
        others = [i for i in range(n) if i != 2]
        assert np.array_equal(again[t][1][others].numpy().astype(np.int64), G["bet_bins"][others, 3 + t])
        assert float(np.abs(again[t][0][others].numpy().astype(np.float64) - G["bet_ref"][others, 3 + t]).max()) < BAR
    assert pol.hist.len.tolist() == [5, 5, 3, 5, 5, 5]


def test_ragged_batch_equals_per_lane_policies():
    """History lengths 1 .. 5 in ONE right-padded batch: every lane gets what a single-environment policy with the same history and the same u computes."""
    n, T = 5, 9
    gen = torch.Generator().manual_seed(21)
    obs = torch.randn(n, T, OBS, generator=gen) * 0.3
    u = torch.rand(n, T, generator=gen)
    pol = golden_policy("cpu", Bank(u))
    restarts = {4: [1], 5: [2], 6: [3], 7: [4]}      # before call 8 the lanes hold 5, 4, 3, 2, 1 observations
    out = []
    for t in range(T):
        if t in restarts:
            m = torch.zeros(n, dtype=torch.uint8); m[restarts[t]] = 1
            pol.begin_episodes(m)
        out.append((pol.predict_batch(obs[:, t]).clone(), pol.last_bins.clone()))
        if t == T - 1:
            assert pol.hist.len.tolist() == [5, 5, 4, 3, 2] and pol.hist.lockstep < 0
        if t == 7:
            assert sorted(pol.hist.len.tolist()) == [1, 2, 3, 4, 5]
    for i in range(n):
        one = golden_policy("cpu", Bank(u[i:i + 1]))
        for t in range(T):
            if t in restarts and i in restarts[t]:
                one.reset()
            a = one.predict_batch(obs[i:i + 1, t])
            assert int(one.last_bins[0]) == int(out[t][1][i]), (i, t)
            np.testing.assert_allclose(a[0].numpy(), out[t][0][i].numpy(), atol=2e-6, err_msg="lane %d step %d" % (i, t))


def _stand_in_agent():
    """An object with the attributes from_reference reads off a live BeT_Agent, carrying the fixture's tensors."""
    sd = golden_sd()
    gpt = types.SimpleNamespace(state_dict=lambda: sd)
    f64 = lambda k: torch.as_tensor(G[k], dtype=torch.float64)
    scaler = types.SimpleNamespace(x_mean=f64("bet_x_mean"), x_std=f64("bet_x_std"), y_mean=f64("bet_y_mean"), y_std=f64("bet_y_std"), y_bounds=G["bet_y_bounds"])
    return types.SimpleNamespace(model=types.SimpleNamespace(model=types.SimpleNamespace(model=gpt, n_head=HEADS)), action_ae=types.SimpleNamespace(bin_centers=torch.as_tensor(G["bet_centers"])),
                                 scaler=scaler, min_action=torch.as_tensor(G["bet_y_bounds"][0]), max_action=torch.as_tensor(G["bet_y_bounds"][1]), window_size=WINDOW,
                                 predict=lambda s: (_ for _ in ()).throw(AssertionError("the batched policy must not call predict")))


def test_from_reference_and_adapter_selection_and_fork():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = _stand_in_agent()
    assert P.BeTPolicy.matches(agent) and not P.BeTPolicy.matches(types.SimpleNamespace(model=torch.nn.Linear(2, 2), predict=None))
    pol = as_batched(agent, 6)
    assert isinstance(pol, P.BeTPolicy) and not isinstance(pol, RowwiseAgent)
    assert isinstance(as_batched(types.SimpleNamespace(predict=lambda s: s), 2), RowwiseAgent)      # anything else still goes row by row
    pol.uniform_fn = Bank(G["bet_u"])
    obs = G["bet_obs"]
    for t in range(3):
        a = pol.predict_batch(torch.as_tensor(obs[:, t]))
        assert np.array_equal(pol.last_bins.numpy().astype(np.int64), G["bet_bins"][:, t])
        assert float(np.abs(a.numpy().astype(np.float64) - G["bet_ref"][:, t]).max()) < BAR
    twin = pol.fork()
    assert twin.trunk is pol.trunk and twin.centers is pol.centers and twin.hist is None and twin._t is not pol._t and int(twin._t) == 3
    twin.uniform_fn = Bank(G["bet_u"])
    twin.predict_batch(torch.as_tensor(obs[:, 0]))
    assert pol.hist.len.tolist() == [3] * 6 and twin.hist.len.tolist() == [1] * 6 and int(pol._t) == 3 and int(twin._t) == 4


def test_host_philox_and_default_draw():
    """Without uniform_fn the CPU tail draws 24 bits of Philox4x32-10 keyed by (seed, env_offset + row, step word, BET_TAG): the known-answer vectors of the
    generator (Random123 kat_vectors: zero and all-ones key / counter), independence of the batch split, and a fresh draw per step."""
    assert [int(x) for x in P.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(x) for x in P.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    u = P.bet_uniforms(7, 100, 64, 3)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) <= 1.0 - 2.0 ** -24 and len(np.unique(u)) == 64
    assert np.array_equal(P.bet_uniforms(7, 0, 164, 3)[100:], u) and not np.array_equal(P.bet_uniforms(7, 100, 64, 4), u)
    obs = torch.as_tensor(G["bet_obs"])
    whole = golden_policy("cpu", seed=5)
    part = golden_policy("cpu", seed=5)
    part.set_rollout_range(2, 3)
    for t in range(3):
        a, b = whole.predict_batch(obs[:, t]), part.predict_batch(obs[2:5, t])
        assert torch.equal(whole.last_u[2:5], part.last_u) and torch.equal(whole.last_bins[2:5], part.last_bins)
        assert float((a[2:5] - b).abs().max()) < 1e-7      # (torch's CPU GEMM rounds a 3-row and a 6-row batch differently; the draw itself is identical)
        assert np.array_equal(whole.last_u.numpy(), P.bet_uniforms(5, 0, 6, t))


def test_nonfinite_hidden_row_gives_bin_minus_one_and_nan_actions():
    pol = golden_policy("cpu", Bank(G["bet_u"]))
    h = torch.randn(4, EMBD, generator=torch.Generator().manual_seed(1))
    clean = pol.tail(h).clone()
    clean_bins = pol.last_bins.clone()
    pol.uniform_fn.call = 0
    h[1, 3], h[3, 0] = float("nan"), float("inf")
    y = pol.tail(h)
    assert pol.last_bins.tolist() == [int(clean_bins[0]), -1, int(clean_bins[2]), -1]
    assert bool(torch.isnan(y[1]).all()) and bool(torch.isnan(y[3]).all()) and torch.equal(y[[0, 2]], clean[[0, 2]])
