"""Diagnostics: per-wave duration vs rare-path counts for late-episode steps (stats build).

--staggered [STEPS]: the episodes staggered as bench.py staggers them (lane i starts (i * 977) % max_steps steps into its episode, one episode length of
untimed steps first), then STEPS steps (default 300): the busy time of every workgroup-step (the longer of its controller and physics waves, 100 MHz ticks),
its mean, median and percentiles, the share of slow workgroup-steps (more than 1.25 x the median) and what they cost over the median, and per step the mean
and the maximum over the 64 workgroups - what a workgroup needs per step against what a dispatch that waits for its slowest workgroup pays."""
import ctypes as C, os, sys, numpy as np, torch
os.environ.setdefault("D3IL_STATS_LIB", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3il_amd import capi
from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
n = 4096
env = ObstacleAvoidanceVecEnv(n, device=0)
L = capi.load()
env.start(); env.reset(); env.policy_begin()
a = torch.zeros(n, 7, dtype=torch.float64, device=env.device)
W = np.zeros((64, 10), dtype=np.uint64)
G = (C.c_uint64 * 32)()
L.d3il_debug_stats(G, 1)
STAGGERED = "--staggered" in sys.argv
names = ["jacobi", "deflate", "general", "newton_it", "finger", "contact", "ls_it", "serve_busy", "ik_busy", "ticks"]   # slot 7: busy ticks of the serving wave (three-wave kernel)
if STAGGERED:
    k = sys.argv.index("--staggered")
    steps = int(sys.argv[k + 1]) if len(sys.argv) > k + 1 and sys.argv[k + 1].isdigit() else 300
    ms = env.max_steps_per_episode
    env.step_count[:n] = (torch.arange(n, device=env.device, dtype=torch.int64) * 977 % ms).to(torch.int32)
    busy = np.zeros((steps, 64))
    for t in range(ms + steps):
        env.policy_action(42, 0, t, a)
        L.d3il_debug_wave_stats(W.ctypes.data_as(C.c_void_p), 64, 1)
        _, _, done, _ = env.step(a)
        L.d3il_debug_wave_stats(W.ctypes.data_as(C.c_void_p), 64, 1)
        env.reset(done); env.policy_begin(done)
        if t >= ms:
            busy[t - ms] = np.maximum(W[:, 8], W[:, 9]) / 100.0      # us
    flat = busy.ravel()
    med = float(np.median(flat))
    slow = flat > 1.25 * med
    print("staggered episodes, %d steps x 64 workgroups, busy us per workgroup-step (diagnostics build): mean %.1f median %.1f p10 %.1f p90 %.1f p99 %.1f max %.1f"
          % (steps, flat.mean(), med, np.percentile(flat, 10), np.percentile(flat, 90), np.percentile(flat, 99), flat.max()))
    print("slow workgroup-steps (> 1.25 x median): %d of %d = %.3f %%, mean excess over the median %.1f us" % (slow.sum(), flat.size, 100.0 * slow.mean(), (flat[slow] - med).mean() if slow.any() else 0.0))
    print("per step: mean over the 64 workgroups %.1f us, maximum over the 64 workgroups mean %.1f median %.1f; over halves of 32: %.1f; steps with a slow workgroup %.1f %%"
          % (busy.mean(), busy.max(1).mean(), np.median(busy.max(1)), 0.5 * (busy[:, :32].max(1).mean() + busy[:, 32:].max(1).mean()), 100.0 * slow.reshape(busy.shape).any(1).mean()))
    print("ratio (mean of the per-step maximum) / (workgroup mean): 64 workgroups %.4f, 32 workgroups %.4f" % (busy.max(1).mean() / busy.mean(), 0.5 * (busy[:, :32].max(1).mean() + busy[:, 32:].max(1).mean()) / busy.mean()))
    sys.exit(0)
for t in range(260):
    env.policy_action(42, 0, t, a)
    L.d3il_debug_wave_stats(W.ctypes.data_as(C.c_void_p), 64, 1)
    _, _, done, _ = env.step(a)
    L.d3il_debug_wave_stats(W.ctypes.data_as(C.c_void_p), 64, 1)
    env.reset(done); env.policy_begin(done)
    if t in (30, 150, 200, 250):
        tot = np.maximum(W[:, 8], W[:, 9])
        order = np.argsort(tot)
        print("t", t, "busy ticks (100 MHz) per workgroup: ik min/med/max", np.min(W[:, 8]), int(np.median(W[:, 8])), np.max(W[:, 8]),
              "| physics min/med/max", np.min(W[:, 9]), int(np.median(W[:, 9])), np.max(W[:, 9]))
        for w in list(order[:2]) + list(order[30:32]) + list(order[-4:]):
            print("   wg %2d ik %7d phys %7d " % (w, W[w, 8], W[w, 9]) + " ".join("%s %d" % (names[i], W[w, i]) for i in (0, 1, 2, 3, 5, 6, 7)))
L.d3il_debug_stats(G, 0)
print("whole run (lane events): deflate solves %d, of which from a warm vector %d, Rayleigh-quotient steps %d (%.2f per deflate solve)" % (G[2], G[25], G[24], G[24] / max(1, G[2])))
