"""Measurement of the batched DDPM-GPT policy (policies.DDPMGPTPolicy): 120 wide / 6 layers / 6 heads, window 5, 8 timesteps, on Stacking
(obs 20 -> 8) and Sorting (obs 16 -> 2) observations.

  python tools/gpu_ddpm_gpt_policy.py [--rows 4096] [--calls 20] [--runs 3] [--out FILE.md]

Per task: ``predict_batch`` ms at ``rows`` environments with a full window for (a) the torch glue (D3IL_POLICY_DDPM_GPT_STEP=0; its normals come from torch.randn on
the device through ``noise_in`` - the host Philox of the fallback would only add a host round trip per chain index that the glue itself does not need) and (b) the
step kernel (Philox inside the kernel), alternating a / b / a / b .. in one process (``runs`` runs of ``calls`` calls each, event pair around a run, median of the
runs); the step kernel's own duration and that of the torch glue of one chain index (event pair around back-to-back calls on one state); and one line for the
agents.RowwiseAgent path - one batch-1 predict per environment and step with a host round trip, what every reference agent without a batched policy gets - on 64
environments.  Prints one JSON line per figure and a markdown table (also written to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3il_amd import policies as P  # noqa: E402
from d3il_amd.agents import RowwiseAgent  # noqa: E402


def timed_calls(pol, obs, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        pol.predict_batch(obs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


class Batch1Agent:
    """The reference protocol on one environment: numpy row in, numpy [1, A] out, its own history - what RowwiseAgent clones per lane."""

    def __init__(self, pol):
        self.pol = pol

    def __copy__(self):
        return Batch1Agent(self.pol.fork())

    def reset(self):
        self.pol.reset()

    def predict(self, row):
        return self.pol.predict_batch(torch.as_tensor(row, device=self.pol.device).reshape(1, -1)).cpu().numpy()


def chain_state(pol, obs):
    """The state dict of one chain (as predict_batch builds it) plus hidden rows, for timing one chain index alone."""
    n, dev, m = obs.shape[0], obs.device, pol.model
    pol.ensure_packed()
    st = dict(x=torch.randn(n, pol.W, pol.A, device=dev), xbuf=torch.randn(n, 2 * pol.W + 1, m.embed_dim, device=dev), actions=torch.empty(n, pol.A, device=dev),
              bad=torch.zeros(n, dtype=torch.int32, device=dev), len=torch.full((n,), pol.W, dtype=torch.int64, device=dev), w=pol._packed.buf)
    return st, torch.randn(n, pol.W, m.embed_dim, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["| task | rows | predict_batch, torch glue (ms) | predict_batch, step kernel (ms) | step kernel alone (us / chain index) | torch glue alone (us / chain index) | RowwiseAgent, 64 envs (ms / step) |",
             "|---|---|---|---|---|---|---|"]
    for task, obs_dim, A in (("stacking", 20, 8), ("sorting", 16, 2)):
        kern = P.DDPMGPTPolicy.random(obs_dim, A, device=dev, seed=1)
        glue = P.DDPMGPTPolicy(kern.model, kern.scaler, kern.T, kern.W, noise_in=lambda k, n, W=kern.W: torch.randn(n, W, A, device=dev))
        pols = {"0": glue, "1": kern}
        obs = torch.randn(args.rows, obs_dim, device=dev) * 0.5
        res = {"0": [], "1": []}
        for mode in ("0", "1"):      # warm-up of both forms, window filled
            os.environ["D3IL_POLICY_DDPM_GPT_STEP"] = mode
            for _ in range(6):
                pols[mode].predict_batch(obs)
        torch.cuda.synchronize()
        for _ in range(args.runs):
            for mode in ("0", "1"):
                os.environ["D3IL_POLICY_DDPM_GPT_STEP"] = mode
                res[mode].append(timed_calls(pols[mode], obs, args.calls))
        os.environ.pop("D3IL_POLICY_DDPM_GPT_STEP", None)
        # one chain index alone, on one state
        alone = {}
        for name, pol in (("kernel", kern), ("torch", glue)):
            st, hk = chain_state(pol, obs)
            fn = pol._step_kernel if name == "kernel" else pol._step_torch
            reps = 200 if name == "kernel" else 50
            for _ in range(5):
                fn(st, 3, hk)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(st, 3, hk)
            e1.record()
            torch.cuda.synchronize()
            alone[name] = e0.elapsed_time(e1) / reps * 1e3
        # the row-by-row adapter on 64 environments
        rw = RowwiseAgent(Batch1Agent(P.DDPMGPTPolicy.random(obs_dim, A, device=dev, seed=1)), 64)
        o64 = obs[:64]
        for _ in range(2):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        row_ms = (time.perf_counter() - t0) / 3 * 1e3
        out = {"task": task, "rows": args.rows, "torch_glue_ms": res["0"], "step_kernel_ms": res["1"], "torch_glue_ms_median": statistics.median(res["0"]),
               "step_kernel_ms_median": statistics.median(res["1"]), "step_kernel_alone_us": alone["kernel"], "torch_glue_alone_us": alone["torch"], "rowwise_64_envs_ms_per_step": row_ms}
        print(json.dumps(out), flush=True)
        lines.append("| %s | %d | %.3f (%s) | %.3f (%s) | %.1f | %.1f | %.1f |" % (task, args.rows, out["torch_glue_ms_median"], ", ".join("%.3f" % v for v in res["0"]),
                                                                                out["step_kernel_ms_median"], ", ".join("%.3f" % v for v in res["1"]), alone["kernel"], alone["torch"], row_ms))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
