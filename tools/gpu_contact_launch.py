"""Avoiding: all rods touch an obstacle in the same step (golden `collide` set-points on every lane, fused rollout step, 1024 environments = one sub-batch of
the default bench): duration of the launches around the contact from the handle's event pair, for the three-wave and the two-wave split kernel.  The launch
after the contact step begins with done = 1 on every lane and resets them in its epilogue.  D3IL_LIB_PATH selects the library."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "oracle_avoiding_rollout.npz"))
COL = GOLD["collide__actions"]
n = 1024
for serve in (256, 0):
    env = ObstacleAvoidanceVecEnv(n, device=0, max_steps_per_episode=250)
    env.set_option("serve_wave_max_workgroups", serve)
    env.set_init_qpos(GOLD["init_qpos"]); env.reset(); env.policy_begin()
    env.set_option("fuse_rollout_tail", 1)
    episodes = torch.zeros(2, dtype=torch.int64, device=env.device)
    actions = torch.zeros(n, 7, dtype=torch.float64, device=env.device)
    env.set_timing(True)
    ms, touching, reset = [], [], []
    for t in range(len(COL) + 6):
        if t:
            actions.copy_(torch.as_tensor(np.repeat(COL[min(t - 1, len(COL) - 1)][None], n, 0), dtype=torch.float64, device=env.device))
        env.random_rollout_step(23, 9000, t, actions, episodes)
        torch.cuda.synchronize()
        ms.append(env.last_step_ms()); touching.append(int(((env.flags[:n] >> 14) & 1).sum())); reset.append(int(env.last_reset.sum()))
    ms = np.array(ms) * 1e3
    tc = next(i for i, k in enumerate(touching) if k)
    print("serve_wave_max_workgroups %d: resting launch (median of steps 10..%d) %.1f us; contact step %d: %.1f us (%d lanes touching afterwards); launch after it: %.1f us (%d lanes reset); next: %.1f us"
          % (serve, tc - 5, float(np.median(ms[10:tc - 4])), tc, ms[tc], touching[tc], ms[tc + 1], reset[tc + 1], ms[tc + 2]))
    print("  us, steps %d..: %s" % (tc - 3, np.round(ms[tc - 3:tc + 5], 1).tolist()))
    env.close()
