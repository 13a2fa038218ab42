"""Link-near guard: the evaluation contexts stay clean (G3).  The set-ups of tests/test_gpu_full_episode_flags.py - 4096 environments, 60 contexts, the
stand-in MLP policy and the scripted pushing policy, full episodes with device auto-reset, the three generic-engine tasks - with BAD = the link-near bit:
in four of the six set-ups no capsule of a robot collision hull the engine does not collide comes within the 2 cm margin of a cube or a static box, so the
unmodelled pairs do not decide any of their episodes.  Two set-ups are NOT clean; the margin was not tuned down, the flagged contexts are
the expected set below (measured on the MI355X with the NumPy reference of tests/link_guard_reference.py on every step):

  Sorting, scripted push, context 24: the policy ends the episode with the arm folded back (TCP x = 0.147); link5's capsule (r = 10.4 cm) comes within 9.3 mm
      of the platform (static box 10) at step 296 and within 2.0 mm at step 298.
  Inserting, stand-in MLP, contexts 3, 6, 51: the random network carries the hand over the gates while the TCP sags to z = 0.07 .. 0.09; context 3: right finger
      capsule 6.8 mm from wall 18 at step 106; context 6: hand capsule 13.9 mm from wall 15 at step 76; context 51: hand capsule 11.6 mm from wall 17 at step
      77, 5.5 mm from wall 15 at step 78.

The same sets are flagged with every margin from 2 cm to 4 cm (5 cm for Inserting), so they do not hang on the last millimetre.  Smallest margin that flags
anything in the clean set-ups (n = 960 sweep): Pushing MLP 5 cm, Pushing scripted 8 cm, Sorting MLP 3 cm (2.5 cm: nothing), Inserting scripted 8 cm."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "ref_offline_ik.npz"))
BAD = 1 << 20
# contexts in which the guard is expected to fire (see the module docstring); every other context must stay clean
EXPECTED = {("pushing", "mlp"): [], ("pushing", "scripted_push"): [], ("sorting", "mlp"): [], ("sorting", "scripted_push"): [24],
            ("inserting", "mlp"): [3, 6, 51], ("inserting", "scripted_push"): []}


def _run(env, pol, steps):
    n = env.n_envs
    env.policy_begin()
    actions = torch.zeros(n, 7, dtype=torch.float64, device=env.device)
    actions[:, 3:] = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=env.device)
    des_xy, des_z = env.policy_des[:2, :n], env.policy_des[2, :n]
    seen = torch.zeros(n, dtype=torch.int32, device=env.device)
    counts = torch.zeros(2, dtype=torch.int64, device=env.device)
    for t in range(steps):
        if hasattr(pol, "begin_episodes"):
            pol.begin_episodes(env.last_reset)
        obs_in = torch.cat((des_xy.t(), env.obs.to(torch.float64)), dim=1)
        des_xy.add_(pol.predict_batch(obs_in).to(torch.float64).t())
        actions[:, 0:2] = des_xy.t()
        actions[:, 2] = des_z
        env.step(actions)
        seen |= env.flags[:n] & BAD             # flags are per episode: collect them before the auto-reset clears them
        env.auto_reset(counts)
    torch.cuda.synchronize()
    st, fl, sc = env.get_state()
    return seen.cpu().numpy(), st, counts.cpu().numpy()


def _check(env, seen, counts, n, ids, expected):
    flagged = np.nonzero(seen)[0]
    print("link-near: %d environments flagged, contexts %s, counter %d, episodes %d" % (len(flagged), sorted(set(ids[flagged].tolist())), env.link_near_episodes, counts[0]))
    assert env.link_guard and env.link_guard_margin == 0.02
    assert sorted(set(ids[flagged].tolist())) == expected, "flagged envs: %d (contexts %s, expected %s)" % (len(flagged), sorted(set(ids[flagged].tolist())), expected)
    assert np.array_equal(seen != 0, np.isin(ids, expected))      # every rollout of an expected context, no other
    assert env.link_near_episodes == len(flagged) and counts[0] >= n


@pytest.mark.parametrize("policy", ["mlp", "scripted_push"])
def test_pushing_4096_envs_all_60_contexts_full_episode(policy):
    from d3il_amd.agents import RandomResidualMLPPolicy, ScriptedPushPolicy
    from d3il_amd.envs.pushing import BlockPushVecEnv
    ctx60 = np.load(os.path.join(ROOT, "d3il_amd", "data", "pushing_test_contexts.npy"))
    n = 4096
    ids = np.arange(n) % 60
    env = BlockPushVecEnv(n, device=0)
    env.set_init_qpos(G["avoiding__traj_last"].copy())
    env.reset(context=ctx60[ids])
    pol = RandomResidualMLPPolicy(input_dim=10, device=env.device) if policy == "mlp" else ScriptedPushPolicy("pushing", device=env.device)
    seen, st, counts = _run(env, pol, 401)
    _check(env, seen, counts, n, ids, EXPECTED[("pushing", policy)])
    env.close()


@pytest.mark.parametrize("policy", ["mlp", "scripted_push"])
def test_sorting_4096_envs_full_episode(policy):
    from d3il_amd.agents import RandomResidualMLPPolicy, ScriptedPushPolicy
    from d3il_amd.envs.sorting import SortingVecEnv, sample_contexts
    n = 4096
    ids = np.arange(n) % 60
    env = SortingVecEnv(n, device=0, max_steps_per_episode=300)
    env.set_init_qpos(G["sorting__traj_last"].copy())
    env.reset(context=sample_contexts(60, 4, seed=0)[ids])
    pol = RandomResidualMLPPolicy(input_dim=16, device=env.device) if policy == "mlp" else ScriptedPushPolicy("sorting", device=env.device)
    seen, st, counts = _run(env, pol, 301)
    _check(env, seen, counts, n, ids, EXPECTED[("sorting", policy)])
    env.close()


@pytest.mark.parametrize("policy", ["mlp", "scripted_push"])
def test_inserting_4096_envs_full_episode(policy):
    from d3il_amd.agents import RandomResidualMLPPolicy, ScriptedPushPolicy
    from d3il_amd.envs.inserting import GateInsertionVecEnv, sample_contexts
    n = 4096
    ids = np.arange(n) % 60
    env = GateInsertionVecEnv(n, device=0, max_steps_per_episode=300)
    env.set_init_qpos(G["avoiding__traj_last"].copy())
    env.reset(context=sample_contexts(60, seed=0)[ids])
    pol = RandomResidualMLPPolicy(input_dim=13, device=env.device) if policy == "mlp" else ScriptedPushPolicy("inserting", device=env.device)
    seen, st, counts = _run(env, pol, 301)
    _check(env, seen, counts, n, ids, EXPECTED[("inserting", policy)])
    env.close()
