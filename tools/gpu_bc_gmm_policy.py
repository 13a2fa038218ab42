"""Measurement of the batched BC-GMM policy (policies.BCGMMPolicy): hidden 128 / 3 blocks (the shipped configs) on the three shapes the reference's
bc_gmm_benchmark.sh scripts name - avoiding obs 4 -> 2, pushing obs 10 -> 2, aligning obs 20 -> 3 - at G = 8 and G = 64 mixture components, low_noise_eval on (the
shipped default).

  python tools/gpu_bc_gmm_policy.py [--rows 4096] [--calls 50] [--runs 5] [--out FILE.md]

Per shape: ``predict_batch`` ms at ``rows`` environments for (a) the policy's own torch path (D3IL_POLICY_BC_GMM_FUSED=0; the draws are device ``torch.rand`` /
``torch.randn`` handed in through ``u_in`` / ``z_in`` - the host Philox of the fallback would add a synchronisation and NumPy work per call that the layers
themselves do not need), (b) the kernel eager (Philox inside) and (c) the kernel under CapturedPolicy, alternating a / b / c / a / b / c .. in one process after a
warm-up of every form (``runs`` runs of ``calls`` calls each, event pair around a run; median and range of the runs); and one line for the agents.RowwiseAgent path -
one batch-1 predict per environment and step through torch's distribution objects as the reference's BC_GMM builds them, a host-to-device copy and a device-to-host
copy, what a BC-GMM agent got before this policy - on 64 environments.  Prints one JSON line per shape and a markdown table (also written to --out)."""
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

SWITCH = "D3IL_POLICY_BC_GMM_FUSED"


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


class Batch1Agent:
    """BC_Agent.predict around BC_GMM.forward(..).sample() on one environment as the reference computes it: numpy row in, torch's own layers on a [1, 1, obs] row,
    Categorical / Independent(Normal) / MixtureSameFamily, one sample, clamp, inverse scaling, numpy [1, A] out."""

    def __init__(self, pol):
        self.pol = pol

    @torch.no_grad()
    def predict(self, row):
        from torch import distributions as D
        p, m = self.pol, self.pol.model
        x = p.scaler.scale_input(torch.from_numpy(row).float().to(p.device).unsqueeze(0).unsqueeze(0))
        for layer in m.mlp.layers:
            x = layer(x)
        f = torch.nn.functional.mish(x)
        means = (0.01 * torch.tanh(m.mean_mlp(f))).reshape(1, 1, p.G, p.A)
        stds = torch.ones_like(means) * 1e-4
        gmm = D.MixtureSameFamily(D.Categorical(logits=m.logits_mlp(f)), D.Independent(D.Normal(loc=means, scale=stds), 1))
        y = gmm.sample().clamp_(p.lo, p.hi)
        return (y * p.out_scale + p.out_shift).detach().cpu().numpy()[0]

    def reset(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    os.environ.pop(SWITCH, None)
    lines = ["| shape | rows | torch path (ms) | kernel eager (ms) | kernel captured (ms) | torch / eager | torch / captured | RowwiseAgent, 64 envs (ms / step) |", "|---|---|---|---|---|---|---|---|"]
    cases = {}
    for task, obs_dim, A in (("avoiding", 4, 2), ("pushing", 10, 2), ("aligning", 20, 3)):
        for G in (8, 64):
            mk = lambda **kw: P.BCGMMPolicy.random(obs_dim, A, device=dev, seed=1, hidden_dim=128, n_blocks=3, n_gaussians=G, **kw)
            kern, inner = mk(), mk()
            layers = mk(u_in=lambda n: torch.rand(n, device=dev), z_in=lambda n, A=A: torch.randn(n, A, device=dev))
            cap = inner.captured()
            obs = torch.randn(args.rows, obs_dim, device=dev) * 0.5
            forms = {"torch": ("0", lambda p=layers, o=obs: p.predict_batch(o)), "eager": ("1", lambda p=kern, o=obs: p.predict_batch(o)),
                     "captured": ("1", lambda p=cap, o=obs: p.predict_batch(o))}
            cases["%s obs %d -> %d, G = %d" % (task, obs_dim, A, G)] = {"forms": forms, "pol": kern, "obs": obs, "res": {k: [] for k in forms}}
    for q in cases.values():      # warm-up of every form (the captured one captures here)
        for mode, fn in q["forms"].values():
            os.environ[SWITCH] = mode
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    for _ in range(args.runs):      # the shapes and the three forms alternate in one process
        for q in cases.values():
            for k, (mode, fn) in q["forms"].items():
                os.environ[SWITCH] = mode
                q["res"][k].append(timed(fn, args.calls))
    os.environ.pop(SWITCH, None)
    for name, q in cases.items():
        rw = RowwiseAgent(Batch1Agent(q["pol"]), 64)
        o64 = q["obs"][:64]
        rw.predict_batch(o64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        row_ms = (time.perf_counter() - t0) / 3 * 1e3
        med = {k: statistics.median(v) for k, v in q["res"].items()}
        out = {"shape": name, "rows": args.rows, "calls": args.calls, "ms": q["res"], "ms_median": med, "torch_over_eager": med["torch"] / med["eager"],
               "torch_over_captured": med["torch"] / med["captured"], "rowwise_64_envs_ms_per_step": row_ms}
        print(json.dumps(out), flush=True)
        cell = lambda k: "%.3f (%.3f .. %.3f)" % (med[k], min(q["res"][k]), max(q["res"][k]))
        lines.append("| %s | %d | %s | %s | %s | %.1f | %.1f | %.1f |" % (name, args.rows, cell("torch"), cell("eager"), cell("captured"), med["torch"] / med["eager"],
                                                                          med["torch"] / med["captured"], row_ms))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
