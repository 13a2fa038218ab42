"""policies.GPTBCPolicy on the CPU against the reference's own Gpt_Agent + GptPolicy + MinGPT + Scaler: tests/golden/ref_gpt_bc_agent.npz holds fixed-seed GPT
weights, a scaler and the reference rolled out batch-1 per environment (6 environments x 8 steps, window 5: it grows, then slides) TWICE - in f32 as shipped and in
f64 (tests/golden/gen_gpt_bc_goldens.py, run where the reference is).  D = max |f32 - f64| of the reference's own actions is the yardstick; the replay must stay
within 4 D of the f64 table.  The device replay of the same fixture is tests/test_gpu_policies_gpt_bc.py."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from d3il_amd import policies as P  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_gpt_bc_agent.npz"))
OBS, EMBD, LAYERS, HEADS, WINDOW, A = (int(v) for v in G["gb_cfg"])
D = float(G["gb_D"][0])
N_ENV, T_STEPS = G["gb_obs"].shape[:2]


def golden_sd():
    return {k[len("gb_sd__"):].replace("__", "."): torch.as_tensor(G[k]) for k in G.files if k.startswith("gb_sd__")}


def golden_policy(dev, seed=0):
    sc = P.Scaler(G["gb_x_mean"], G["gb_x_std"], G["gb_y_mean"], G["gb_y_std"], G["gb_y_bounds"], device=dev)
    trunk = P.MinGPTTrunk(OBS, EMBD, LAYERS, HEADS, WINDOW, vocab_size=A, action_dim=0)
    trunk.load_state_dict(golden_sd())      # the reference's GPT state dict loads as it is
    trunk = trunk.to(dev)
    for p in trunk.parameters():
        p.requires_grad_(False)
    return P.GPTBCPolicy(trunk, sc, WINDOW, seed=seed)


def replay(dev):
    """Worst deviation of the golden replay on ``dev`` (all environments as one batch) from the f64 table, and the policy."""
    pol = golden_policy(dev)
    obs = G["gb_obs"]
    worst = 0.0
    for t in range(T_STEPS):
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(a - G["gb_ref64"][:, t]).max()))
        assert not bool(pol.last_bad.any())
    return worst, pol


def test_policy_rows_equal_reference_predict():
    assert float(np.abs(G["gb_ref32"] - G["gb_ref64"]).max()) == D and G["gb_ref64"].shape == (6, 8, A) and D > 0 and T_STEPS > WINDOW
    lo, hi = G["gb_y_bounds"]
    hit = (G["gb_raw64"] < lo) | (G["gb_raw64"] > hi)
    assert 0 < hit.sum() < hit.size      # some but not all outputs reach the action clamp
    worst, pol = replay("cpu")
    print("golden replay (cpu): actions %.3e = %.2f D (D %.3e)" % (worst, worst / D, D))
    assert worst <= 4 * D
    assert int(pol._t) == T_STEPS      # no random numbers, but the step word advances


def test_restarted_lanes_and_ragged_batches():
    """Lanes restarted one by one (begin_episodes) run with different window lengths in one right-padded batch: lane e, restarted at step e, must give what the
    reference gave its environment e from its step 0 on - the golden table shifted by e."""
    pol = golden_policy("cpu")
    obs = torch.as_tensor(G["gb_obs"])
    steps = T_STEPS + N_ENV - 1
    worst = 0.0
    for s in range(steps):
        if 0 < s < N_ENV:      # lane s starts its trajectory now; lanes < s are further on, lanes > s run on throwaway rows until their turn
            mask = torch.zeros(N_ENV, dtype=torch.bool)
            mask[s] = True
            pol.begin_episodes(mask)
        t = [min(max(s - e, 0), T_STEPS - 1) for e in range(N_ENV)]
        a = pol.predict_batch(torch.stack([obs[e, t[e]] for e in range(N_ENV)])).numpy().astype(np.float64)
        for e in range(N_ENV):
            if 0 <= s - e < T_STEPS:
                worst = max(worst, float(np.abs(a[e] - G["gb_ref64"][e, s - e]).max()))
    lens = pol.hist.padded()[1].tolist()
    assert lens == [WINDOW] * N_ENV
    print("ragged replay (cpu): actions %.3e = %.2f D" % (worst, worst / D))
    assert worst <= 4 * D
    # reset() empties every window: the first rows again
    pol.reset()
    a = pol.predict_batch(obs[:, 0]).numpy().astype(np.float64)
    assert float(np.abs(a - G["gb_ref64"][:, 0]).max()) <= 4 * D


# ---- duck-typed reference agents (class names as in the reference: matches() goes by them)
class _GPT(torch.nn.Module):
    def __init__(self, head_bias=False, rows=A, discrete=False):
        super().__init__()
        self.inner = P.MinGPTTrunk(OBS, EMBD, LAYERS, HEADS, WINDOW, vocab_size=rows, action_dim=0)
        if head_bias:
            self.inner.head = torch.nn.Linear(EMBD, rows, bias=True)
        if discrete:
            self.inner.tok_emb = torch.nn.Embedding(OBS, EMBD)

    def state_dict(self, *a, **k):
        return self.inner.state_dict(*a, **k)


class MinGPT(torch.nn.Module):
    def __init__(self, **kw):
        super().__init__()
        self.model = _GPT(**kw)
        self.n_head = HEADS


class GptPolicy(torch.nn.Module):
    def __init__(self, encoder=None, visual_input=False, **kw):
        super().__init__()
        self.model = MinGPT(**kw)
        self.obs_encoder = encoder if encoder is not None else torch.nn.Identity()
        self.visual_input = visual_input


class Gpt_Agent:
    def __init__(self, model=None, load=True, window=WINDOW, bounds=None):
        self.model = model or GptPolicy()
        self.scaler = types.SimpleNamespace(x_mean=torch.as_tensor(G["gb_x_mean"]), x_std=torch.as_tensor(G["gb_x_std"]), y_mean=torch.as_tensor(G["gb_y_mean"]),
                                            y_std=torch.as_tensor(G["gb_y_std"]), y_bounds=G["gb_y_bounds"] if bounds is None else bounds)
        self.min_action, self.max_action = torch.as_tensor(G["gb_y_bounds"][0]), torch.as_tensor(G["gb_y_bounds"][1])
        self.window_size = window
        if load:
            self.model.model.model.inner.load_state_dict(golden_sd())

    def predict(self, s):
        return np.zeros(A)

    def reset(self):
        pass


class BC_Agent(Gpt_Agent):
    pass


def test_from_reference_and_adapter_selection():
    from d3il_amd.agents import RowwiseAgent, as_batched
    from tests.test_policies_bet_mlp import BetMLP_Agent, _real_bet_agent
    agent = Gpt_Agent()
    assert P.GPTBCPolicy.matches(agent)
    assert not any(c.matches(agent) for c in (P.BeTPolicy, P.BeTMLPPolicy, P.CVAEPolicy, P.IBCPolicy, P.ACTPolicy, P.DDPMGPTPolicy, P.DDPMACTPolicy))
    assert P.GPTBCPolicy.matches(Gpt_Agent(window=1))
    others = {"a head with bias": Gpt_Agent(GptPolicy(head_bias=True), load=False), "visual input": Gpt_Agent(GptPolicy(visual_input=True)),
              "an observation encoder": Gpt_Agent(GptPolicy(encoder=torch.nn.Linear(OBS, OBS))), "discrete input": Gpt_Agent(GptPolicy(discrete=True), load=False),
              "bounds of another width": Gpt_Agent(bounds=np.zeros((2, A + 1))), "no bounds": Gpt_Agent(bounds=False), "a window beyond the block size": Gpt_Agent(window=WINDOW + 1),
              "another agent class": BC_Agent()}
    others["no bounds"].scaler.y_bounds = None
    for name, other in others.items():
        assert not P.GPTBCPolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    # the BeT agents stay where they are, and the reverse
    bet, bet_mlp = _real_bet_agent(), BetMLP_Agent()
    assert not P.GPTBCPolicy.matches(bet) and not P.GPTBCPolicy.matches(bet_mlp)
    assert type(as_batched(bet, 2)) is P.BeTPolicy and type(as_batched(bet_mlp, 2)) is P.BeTMLPPolicy
    pol = as_batched(agent, 4)
    assert type(pol) is P.GPTBCPolicy and pol.A == A and pol.W == WINDOW and pol.trunk.n_embd == EMBD and pol.trunk.head.bias is None
    assert np.array_equal(pol.min_action.numpy(), G["gb_y_bounds"][0].astype(np.float32)) and np.array_equal(pol.max_action.numpy(), G["gb_y_bounds"][1].astype(np.float32))
    a = pol.predict_batch(torch.as_tensor(G["gb_obs"][:, 0])).numpy().astype(np.float64)
    assert float(np.abs(a - G["gb_ref64"][:, 0]).max()) <= 4 * D
    # fork: trunk shared, step word its own, an empty window
    twin = pol.fork()
    assert twin.trunk is pol.trunk and twin._t is not pol._t and int(twin._t) == int(pol._t) == 1 and twin.hist is None and twin.last_bad is None
    b = twin.predict_batch(torch.as_tensor(G["gb_obs"][:, 0])).numpy().astype(np.float64)
    assert np.array_equal(a, b) and int(twin._t) == 2 and int(pol._t) == 1
    # a sub-batch is a slice of the whole (no random numbers: set_rollout_range only sizes the window)
    part = golden_policy("cpu")
    part.set_rollout_range(2, 3)
    c = part.predict_batch(torch.as_tensor(G["gb_obs"][2:5, 0])).numpy().astype(np.float64)
    assert part.env_offset == 2 and float(np.abs(c - a[2:5]).max()) <= 4 * D


def test_nonfinite_inputs_mark_their_environment_only():
    clean, dirty = golden_policy("cpu"), golden_policy("cpu")
    obs = torch.as_tensor(G["gb_obs"])
    for t in range(2):
        want = clean.predict_batch(obs[:, t])
        o = obs[:, t].clone()
        if t == 1:
            o[2, 1], o[4, 0] = float("nan"), float("inf")
        have = dirty.predict_batch(o)
    good = [0, 1, 3, 5]
    assert torch.isfinite(want).all()
    assert torch.isnan(have[[2, 4]]).all() and torch.equal(have[good], want[good])
    assert dirty.last_bad.tolist() == [0, 0, 1, 0, 1, 0] and not bool(clean.last_bad.any())
    # the bad observation stays in the lane's window until it slides out or the lane restarts
    mask = torch.zeros(N_ENV, dtype=torch.bool)
    mask[2] = True
    dirty.begin_episodes(mask)
    have = dirty.predict_batch(obs[:, 2])
    assert torch.isfinite(have[2]).all() and torch.isnan(have[4]).all()


def test_binding_has_the_headers_argument_list():
    """capi's argtypes of d3il_gpt_bc_head_f32 against the declaration in include/d3il_rollout.h: count and kind (pointer / float / long / int) of every argument."""
    import ctypes as C
    import re
    from d3il_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "d3il_rollout.h")).read()
    decl = re.search(r"int d3il_gpt_bc_head_f32\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kind = lambda a: C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_uint64 if a.startswith("uint64_t") else C.c_long if a.startswith("long") else C.c_int
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "ln_weight", "ln_bias", "ln_eps", "w_head", "lo", "hi", "scale", "shift", "actions", "bad", "rows", "C", "A", "stream"]
    assert capi.load().d3il_gpt_bc_head_f32.argtypes == [kind(a) for a in args]
    assert "d3il_gpt_bc_head_f32" in capi.EXPORTS and P.GPTBCPolicy.SWITCH == "D3IL_POLICY_GPT_BC_HEAD"
    assert capi.load().d3il_version() == 2
