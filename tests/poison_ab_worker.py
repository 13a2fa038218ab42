"""Worker of tests/test_gpu_poison_build.py: one child process per library (D3IL_LIB_PATH names it; unset = the product library).

    python tests/poison_ab_worker.py episodes <outdir>     one deterministic episode per task -> <outdir>/<task>.npy ([steps][rows + 1][n]: states, flags)
    python tests/poison_ab_worker.py control <outdir>      the positive control -> <outdir>/control.json

The episodes are those of tests/test_gpu_permutation.py (same seeds and policies, 256 environments): Avoiding open loop with a drift towards the
obstacles - once with the serving wave and once in the two-wave form -, Pushing / Sorting / Inserting closed loop on scripted policies that reach
rod <-> cube, cube <-> cube and wall contacts.  The caller compares what two libraries wrote, bit for bit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3il_amd import capi  # noqa: E402

N = 256
SOLVER_FAIL = 1 << 16


def build_flags():
    out = np.zeros(8, dtype=np.int32)
    capi.check(capi.load().d3il_debug_build_flags(out.ctypes.data_as(C.c_void_p)))
    return out


def avoiding_episode(two_wave, steps=150):
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    rng = np.random.default_rng(3)
    delta = rng.uniform(-0.01, 0.01, size=(steps, N, 2)) + np.array([0.0, 0.004])
    env = ObstacleAvoidanceVecEnv(N, device=0)
    if two_wave:
        env.set_option("serve_wave_max_workgroups", 0)
    env.start()
    env.reset()
    rs = env.robot_state()
    des, z = rs[:, :2].clone(), rs[:, 2:3].clone()
    quat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=des.device).expand(N, 4)
    out = []
    for t in range(steps):
        des = des + torch.as_tensor(delta[t], dtype=torch.float64, device=des.device)
        env.step(torch.cat((des, z, quat), dim=1).contiguous())
        torch.cuda.synchronize()
        st, fl, _ = env.get_state()
        out.append(np.concatenate([st, fl[None].astype(np.float64)], axis=0))
    env.close()
    return np.stack(out)


def contact_episode(task, steps):
    from d3il_amd.agents import ScriptedGoalPushPolicy, ScriptedPushPolicy
    rng = np.random.default_rng(5)
    if task == "inserting":
        from d3il_amd.envs.inserting import GateInsertionVecEnv as Env, sample_contexts
        ctx, plan = sample_contexts(N, seed=5), None
    elif task == "pushing":
        from d3il_amd.envs.pushing import BlockPushVecEnv as Env, sample_contexts
        ctx, plan = sample_contexts(N, seed=5), rng.integers(0, 4, size=N)
    else:
        from d3il_amd.envs.sorting import SortingVecEnv as Env, sample_contexts
        ctx, plan = sample_contexts(N, 4, seed=5).reshape(N, -1), None
    env = Env(N, device=0)
    env.start()
    obs = env.reset(random=False, context=ctx)
    dev = obs.device
    pol = ScriptedPushPolicy(task, device=dev) if task == "inserting" else ScriptedGoalPushPolicy(task, plan=plan, device=dev)
    rs = env.robot_state()
    des, z = rs[:, :2].clone(), rs[:, 2:3].clone()
    quat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=dev).expand(N, 4)
    out = []
    for t in range(steps):
        des = des + pol.predict_batch(torch.cat((des, obs.to(torch.float64)), dim=1))
        obs, _, done, info = env.step(torch.cat((des, z, quat), dim=1).contiguous())
        torch.cuda.synchronize()
        st, fl, _ = env.get_state()
        out.append(np.concatenate([st, fl[None].astype(np.float64)], axis=0))
    env.close()
    return np.stack(out)


def control():
    """Sorting, four cubes well apart, the set-point held at the start pose until the cubes rest on the platform; then one environment's record area."""
    from d3il_amd.envs.sorting import SortingVecEnv
    from tests.test_sorting_oracle import CTX
    n = 32
    env = SortingVecEnv(n, device=0)
    env.start()
    env.reset(random=False, context=np.tile(CTX.reshape(1, -1), (n, 1)))
    rs = env.robot_state()
    quat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=rs.device).expand(n, 4)
    act = torch.cat((rs[:, :3].clone(), quat), dim=1).contiguous()
    for t in range(40):      # the cubes hop for about 14 steps after a reset (tests/test_sorting_host.py::test_reset_and_hop)
        env.step(act)
    torch.cuda.synchronize()
    st, fl, _ = env.get_state()
    bf = build_flags()
    gg, seg, grec, maxnb = int(bf[1]), int(bf[2]), int(bf[3]), int(bf[4])
    areas = []
    for e in (5, 21):      # two workgroups
        buf = np.zeros(gg)
        capi.check(env.L.d3il_debug_scratch(env.h, e, buf.ctypes.data_as(C.c_void_p), gg))
        areas.append(buf)
    env.close()
    vel = float(np.abs(np.concatenate([st[42 + 13 * b + 7:42 + 13 * b + 13] for b in range(4)])).max())
    moved_xy = float(max(np.abs(st[42 + 13 * b:44 + 13 * b, :] - CTX[b, :2, None]).max() for b in range(4)))
    res = dict(build_flags=int(bf[0]), gg=gg, seg=seg, grec=grec, maxnb=maxnb, max_cube_speed=vel, cube_xy_drift=moved_xy,
               flags_or=int(np.bitwise_or.reduce(fl)), state_finite=bool(np.isfinite(st).all()), envs=[])
    for buf in areas:
        r = buf.reshape(maxnb + 1, seg, grec)
        res["envs"].append(dict(finite_mask_record0=[np.isfinite(r[b, 0]).astype(int).tolist() for b in range(4)],
                                last_record_nan=[int(np.isnan(r[b, seg - 1]).sum()) for b in range(4)],
                                arm_segment_nan=int(np.isnan(r[maxnb]).sum()), nan_total=int(np.isnan(buf).sum()),
                                finite_records=[int(np.isfinite(r[b, :, :16]).all(axis=1).sum()) for b in range(maxnb + 1)]))
    return res


def main():
    mode, outdir = sys.argv[1], sys.argv[2]
    os.makedirs(outdir, exist_ok=True)
    if mode == "control":
        with open(os.path.join(outdir, "control.json"), "w") as f:
            json.dump(control(), f)
        return
    assert mode == "episodes"
    with open(os.path.join(outdir, "build.json"), "w") as f:
        json.dump(dict(build_flags=int(build_flags()[0])), f)
    np.save(os.path.join(outdir, "avoiding.npy"), avoiding_episode(False))
    np.save(os.path.join(outdir, "avoiding_two_wave.npy"), avoiding_episode(True))
    for task, steps in (("pushing", 220), ("sorting", 300), ("inserting", 260)):
        np.save(os.path.join(outdir, task + ".npy"), contact_episode(task, steps))


if __name__ == "__main__":
    main()
