"""Measurement of the batched VAE-ACT policy (policies.ACTPolicy) on the shipped shape: 2 encoder and 4 decoder layers, width 64, 4 heads,
latent 32, chunks of 3, obs 10 -> 2.

  python tools/gpu_act_policy.py [--rows 4096] [--calls 20] [--runs 3] [--out FILE.md]

``predict_batch`` ms at ``rows`` environments for (a) the torch path (D3IL_POLICY_ACT_FUSED=0; its latent comes from torch.rand on the device through ``latent_in``,
so that the host Philox of the fallback is not in its time) and (b) the chunk kernel (Philox inside), alternating a / b / a / b .. in one process (``runs`` runs of
``calls`` calls each, an event pair around a run, median of the runs), in two regimes:
  * every lane due on every call (``reset()`` before each call, on both paths);
  * the lock-step steady state: all lanes share a chunk phase, one call in T computes.
And one line for the agents.RowwiseAgent path - one batch-1 predict per environment and step with a host round trip, what an ActAgent got before this policy - on 64
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


def timed_calls(pol, obs, calls, all_due):
    pol.reset()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        if all_due:
            pol.reset()
        pol.predict_batch(obs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


class Batch1Agent:
    """ActAgent.predict on one environment as the reference computes it: numpy row in, a batch-1 forward of torch's own layers every T steps, numpy [1, A] out."""

    def __init__(self, pol):
        self.pol, self.counter, self.chunk = pol, pol.T, None

    def reset(self):
        self.counter = self.pol.T

    def predict(self, row):
        p = self.pol
        if self.counter == p.T:
            self.counter = 0
            s = p.scaler.scale_input(torch.as_tensor(row, dtype=torch.float32, device=p.device).reshape(1, -1))
            self.chunk = p._chunk_torch(s, torch.rand(1, 32, device=p.device))
        a = self.chunk[:, self.counter]
        self.counter += 1
        return a.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kern = P.ACTPolicy.random(10, 2, 3, device=dev, seed=1, n_envs=args.rows)
    plain = P.ACTPolicy(kern.model, kern.scaler, n_envs=args.rows, latent_in=lambda n: torch.rand(n, 32, device=dev))
    pols, obs = {"0": plain, "1": kern}, torch.randn(args.rows, 10, device=dev) * 0.5
    res = {(m, r): [] for m in ("0", "1") for r in ("all due", "lock-step")}
    for mode in ("0", "1"):      # warm-up of both forms
        os.environ["D3IL_POLICY_ACT_FUSED"] = mode
        for _ in range(4):
            pols[mode].predict_batch(obs)
    torch.cuda.synchronize()
    for _ in range(args.runs):      # the two regimes and the two forms alternate in one process
        for regime in ("all due", "lock-step"):
            for mode in ("0", "1"):
                os.environ["D3IL_POLICY_ACT_FUSED"] = mode
                res[(mode, regime)].append(timed_calls(pols[mode], obs, args.calls, regime == "all due"))
    os.environ.pop("D3IL_POLICY_ACT_FUSED", None)
    rw = RowwiseAgent(Batch1Agent(kern), 64)
    o64 = obs[:64]
    rw.predict_batch(o64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(6):
        rw.predict_batch(o64)
    torch.cuda.synchronize()
    row_ms = (time.perf_counter() - t0) / 6 * 1e3
    lines = ["| regime | rows | predict_batch, torch path (ms) | predict_batch, kernel (ms) | ratio |", "|---|---|---|---|---|"]
    for regime in ("all due", "lock-step"):
        a, b = res[("0", regime)], res[("1", regime)]
        ma, mb = statistics.median(a), statistics.median(b)
        print(json.dumps({"regime": regime, "rows": args.rows, "calls": args.calls, "torch_path_ms": a, "kernel_ms": b, "torch_path_ms_median": ma, "kernel_ms_median": mb}), flush=True)
        lines.append("| %s | %d | %.3f (%s) | %.3f (%s) | %.1f |" % (regime, args.rows, ma, ", ".join("%.3f" % v for v in a), mb, ", ".join("%.3f" % v for v in b), ma / mb))
    print(json.dumps({"rowwise_64_envs_ms_per_step": row_ms}), flush=True)
    lines += ["", "RowwiseAgent (batch-1 predict per environment, a forward every 3 steps), 64 environments: %.1f ms per step" % row_ms]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
