"""Measurement of the batched DDPM-ACT policy (policies.DDPMACTPolicy) on the shipped shape: 2 encoder and 4 decoder layers, width 64, 4 heads,
obs_seq_len 5, chunks of 4, 16 timesteps, obs 10 -> 2.

  python tools/gpu_ddpm_act_policy.py [--rows 4096] [--calls 20] [--runs 3] [--out FILE.md]

``predict_batch`` ms at ``rows`` environments for (a) the torch path (D3IL_POLICY_DDPM_ACT_FUSED=0; its normals come from torch.randn on the device through
``noise_in``, so that the host Philox of the fallback is not in its time) and (b) the chain kernel (Philox inside), alternating a / b / a / b .. in one process
(``runs`` runs of ``calls`` calls each, an event pair around a run, median of the runs), on full windows (L = 5), in three regimes:
  * every lane due on every call (the counters are set to the chunk length before each call, on both paths);
  * the lock-step steady state: all lanes share a chunk phase, one call in 4 computes;
  * staggered episodes: lane i is in phase i mod 4, so a quarter of the lanes - at least one in every 16-lane tile - is due on every call.
And one line for the agents.RowwiseAgent path - one batch-1 predict per environment and step with a host round trip, what an enc-dec DiffusionAgent got before this
policy - on 64 environments.  Prints one JSON line per figure and a markdown table (also written to --out)."""
import argparse
import json
import os
import statistics
import sys
import time
from collections import deque

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3il_amd import policies as P  # noqa: E402
from d3il_amd.agents import RowwiseAgent  # noqa: E402

REGIMES = ("all due", "lock-step", "staggered")


def timed_calls(pol, obs, calls, regime):
    n = obs.shape[0]
    pol.counter.fill_(pol.Ta)
    if regime == "staggered":
        pol.counter.copy_((1 + torch.arange(n, device=obs.device) % pol.Ta).to(torch.int32))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        if regime == "all due":
            pol.counter.fill_(pol.Ta)
        pol.predict_batch(obs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


class Batch1Agent:
    """DiffusionAgent.predict of the enc-dec agent on one environment as the reference computes it: numpy row in, the window deque, a batch-1 chain through torch's
    own layers every 4 steps, numpy [1, A] out."""

    def __init__(self, pol):
        self.pol, self.counter, self.chunk, self.ctx = pol, pol.Ta, None, deque(maxlen=pol.S)

    def reset(self):
        self.counter = self.pol.Ta
        self.ctx.clear()

    def predict(self, row):
        p = self.pol
        self.ctx.append(p.scaler.scale_input(torch.as_tensor(row, dtype=torch.float32, device=p.device).reshape(1, -1)))
        if self.counter == p.Ta:
            self.counter = 0
            self.chunk = p._chain_torch(torch.stack(tuple(self.ctx), dim=1), torch.randn(1, p.T + 1, p.Ta, p.A, device=p.device))[0]
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
    kern = P.DDPMACTPolicy.random(10, 2, device=dev, seed=1, n_envs=args.rows)
    plain = P.DDPMACTPolicy(kern.model, kern.scaler, kern.T, n_envs=args.rows, noise_in=lambda n: torch.randn(n, kern.T + 1, kern.Ta, kern.A, device=dev))
    pols, obs = {"0": plain, "1": kern}, torch.randn(args.rows, 10, device=dev) * 0.5
    res = {(m, r): [] for m in ("0", "1") for r in REGIMES}
    for mode in ("0", "1"):      # warm-up of both forms; the windows fill up (L = 5 from here on)
        os.environ["D3IL_POLICY_DDPM_ACT_FUSED"] = mode
        for _ in range(6):
            pols[mode].predict_batch(obs)
    torch.cuda.synchronize()
    for _ in range(args.runs):      # the regimes and the two forms alternate in one process
        for regime in REGIMES:
            for mode in ("0", "1"):
                os.environ["D3IL_POLICY_DDPM_ACT_FUSED"] = mode
                res[(mode, regime)].append(timed_calls(pols[mode], obs, args.calls, regime))
    os.environ.pop("D3IL_POLICY_DDPM_ACT_FUSED", None)
    rw = RowwiseAgent(Batch1Agent(kern), 64)
    o64 = obs[:64]
    rw.predict_batch(o64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(8):
        rw.predict_batch(o64)
    torch.cuda.synchronize()
    row_ms = (time.perf_counter() - t0) / 8 * 1e3
    lines = ["| regime | rows | predict_batch, torch path (ms) | predict_batch, kernel (ms) | ratio |", "|---|---|---|---|---|"]
    for regime in REGIMES:
        a, b = res[("0", regime)], res[("1", regime)]
        ma, mb = statistics.median(a), statistics.median(b)
        print(json.dumps({"regime": regime, "rows": args.rows, "calls": args.calls, "torch_path_ms": a, "kernel_ms": b, "torch_path_ms_median": ma, "kernel_ms_median": mb}), flush=True)
        lines.append("| %s | %d | %.3f (%s) | %.3f (%s) | %.1f |" % (regime, args.rows, ma, ", ".join("%.3f" % v for v in a), mb, ", ".join("%.3f" % v for v in b), ma / mb))
    print(json.dumps({"rowwise_64_envs_ms_per_step": row_ms}), flush=True)
    lines += ["", "RowwiseAgent (batch-1 predict per environment, a 16-step chain every 4 steps), 64 environments: %.1f ms per step" % row_ms]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
