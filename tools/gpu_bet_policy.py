"""Measurement of the batched BeT policy (policies.BeTPolicy): a 120 / 6 layers / 6 heads trunk, window 5, on Stacking (obs 20 -> 8) and Sorting-4
(obs 16 -> 2) observations.

  python tools/gpu_bet_policy.py [--rows 4096] [--calls 100] [--runs 3] [--out FILE.md]

Per task: ``predict_batch`` ms at ``rows`` environments with a full window for (a) the torch tail (D3IL_POLICY_BET_HEAD=0) and (b) the head kernel, alternating a / b /
a / b .. in one process (``runs`` runs of ``calls`` calls each, event pair around a run, median of the runs); the head kernel's own duration (event pair around 200 back-to-back
launches on one hidden batch); and one line for the agents.RowwiseAgent path - one batch-1 predict per environment and step with a host round trip, what every reference
agent without a batched policy gets - on 64 environments.  Prints one JSON line per figure and a markdown table (also written to --out)."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["| task | rows | predict_batch, torch tail (ms) | predict_batch, head kernel (ms) | head kernel alone (us) | torch tail alone (us) | RowwiseAgent, 64 envs (ms / step) |", "|---|---|---|---|---|---|---|"]
    for task, obs_dim, A in (("stacking", 20, 8), ("sorting", 16, 2)):
        pol = P.BeTPolicy.random(obs_dim, A, device=dev, seed=1)
        obs = torch.randn(args.rows, obs_dim, device=dev) * 0.5
        res = {"0": [], "1": []}
        for mode in ("0", "1"):      # warm-up of both tails, window filled
            os.environ["D3IL_POLICY_BET_HEAD"] = mode
            for _ in range(8):
                pol.predict_batch(obs)
        torch.cuda.synchronize()
        for _ in range(args.runs):
            for mode in ("0", "1"):
                os.environ["D3IL_POLICY_BET_HEAD"] = mode
                res[mode].append(timed_calls(pol, obs, args.calls))
        os.environ.pop("D3IL_POLICY_BET_HEAD", None)
        # the tail alone, on one hidden batch
        h = torch.randn(args.rows, 120, device=dev)
        alone = {}
        for name, fn in (("kernel", pol._tail_kernel), ("torch", pol._tail_torch)):
            reps = 200 if name == "kernel" else 50
            for _ in range(5):
                fn(h)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(h)
            e1.record()
            torch.cuda.synchronize()
            alone[name] = e0.elapsed_time(e1) / reps * 1e3
        # the row-by-row adapter on 64 environments
        rw = RowwiseAgent(Batch1Agent(P.BeTPolicy.random(obs_dim, A, device=dev, seed=1)), 64)
        o64 = obs[:64]
        for _ in range(2):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        row_ms = (time.perf_counter() - t0) / 3 * 1e3
        out = {"task": task, "rows": args.rows, "torch_tail_ms": res["0"], "head_kernel_ms": res["1"], "torch_tail_ms_median": statistics.median(res["0"]),
               "head_kernel_ms_median": statistics.median(res["1"]), "head_kernel_alone_us": alone["kernel"], "torch_tail_alone_us": alone["torch"], "rowwise_64_envs_ms_per_step": row_ms}
        print(json.dumps(out))
        lines.append("| %s | %d | %.3f (%s) | %.3f (%s) | %.1f | %.1f | %.1f |" % (task, args.rows, out["torch_tail_ms_median"], ", ".join("%.3f" % v for v in res["0"]),
                                                                                out["head_kernel_ms_median"], ", ".join("%.3f" % v for v in res["1"]), alone["kernel"], alone["torch"], row_ms))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
