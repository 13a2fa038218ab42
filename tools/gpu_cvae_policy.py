"""Measurement of the batched CVAE policy (policies.CVAEPolicy): hidden 128 / 3 blocks on Avoiding-like observations (obs 4, latent 32 -> 2) and
hidden 256 / 4 blocks on Stacking-like ones (obs 20, latent 16 -> 8).

  python tools/gpu_cvae_policy.py [--rows 4096] [--calls 20] [--runs 3] [--out FILE.md]

Per shape: ``predict_batch`` ms at ``rows`` environments for (a) torch's layers (D3IL_POLICY_CVAE_FUSED=0; the latent is a device ``torch.randn`` handed in through
``z_in`` - the host Philox of the fallback would add a synchronisation and NumPy work per call that the layers themselves do not need) and (b) the kernel (Philox
inside), alternating a / b / a / b .. in one process (``runs`` runs of ``calls`` calls each, event pair around a run, median of the runs); and one line for the
agents.RowwiseAgent path - one batch-1 predict per environment and step with a host ``torch.randn``, a host-to-device copy and a device-to-host copy, what a
CVAEAgent got before this policy - on 64 environments.  Prints one JSON line per figure and a markdown table (also written to --out)."""
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
    """CVAEAgent.predict on one environment as the reference computes it: numpy row in, a host torch.randn copied to the device and clamped, torch's own layers,
    clamp, inverse scaling, numpy [1, A] out."""

    def __init__(self, pol):
        self.pol = pol

    @torch.no_grad()
    def predict(self, row):
        p = self.pol
        s = p.scaler.scale_input(torch.from_numpy(row).float().to(p.device).unsqueeze(0))
        z = torch.randn((1, p.L)).to(p.device).clamp(-0.5, 0.5)
        x = torch.cat([s, z], dim=-1)
        for layer in p.model.layers:
            x = layer(x)
        x = x.clamp_(p.lo, p.hi)
        return (x * p.out_scale + p.out_shift).detach().cpu().numpy()

    def reset(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["| shape | rows | predict_batch, torch's layers (ms) | predict_batch, kernel (ms) | torch / kernel | RowwiseAgent, 64 envs (ms / step) |", "|---|---|---|---|---|---|"]
    shapes = (("hidden 128 / 3 blocks, obs 4 + latent 32 -> 2", 4, 32, 2, 128, 3), ("hidden 256 / 4 blocks, obs 20 + latent 16 -> 8", 20, 16, 8, 256, 4))
    pols = {}
    for name, obs_dim, L, A, hidden, nb in shapes:
        kern = P.CVAEPolicy.random(obs_dim, A, device=dev, seed=1, hidden_dim=hidden, n_blocks=nb, latent_dim=L)
        layers = P.CVAEPolicy(kern.model, kern.scaler, L, z_in=lambda n, L=L: torch.randn(n, L, device=dev))
        pols[name] = {"0": layers, "1": kern, "obs": torch.randn(args.rows, obs_dim, device=dev) * 0.5, "res": {"0": [], "1": []}}
    for name in pols:      # warm-up of both forms
        for mode in ("0", "1"):
            os.environ["D3IL_POLICY_CVAE_FUSED"] = mode
            for _ in range(2):
                pols[name][mode].predict_batch(pols[name]["obs"])
    torch.cuda.synchronize()
    for _ in range(args.runs):      # the two shapes and the two forms alternate in one process
        for name in pols:
            for mode in ("0", "1"):
                os.environ["D3IL_POLICY_CVAE_FUSED"] = mode
                pols[name]["res"][mode].append(timed_calls(pols[name][mode], pols[name]["obs"], args.calls))
    os.environ.pop("D3IL_POLICY_CVAE_FUSED", None)
    for name, obs_dim, L, A, hidden, nb in shapes:
        q = pols[name]
        rw = RowwiseAgent(Batch1Agent(q["1"]), 64)
        o64 = q["obs"][:64]
        rw.predict_batch(o64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        row_ms = (time.perf_counter() - t0) / 3 * 1e3
        med = {m: statistics.median(q["res"][m]) for m in ("0", "1")}
        out = {"shape": name, "rows": args.rows, "torch_layers_ms": q["res"]["0"], "kernel_ms": q["res"]["1"], "torch_layers_ms_median": med["0"], "kernel_ms_median": med["1"],
               "torch_over_kernel": med["0"] / med["1"], "rowwise_64_envs_ms_per_step": row_ms}
        print(json.dumps(out), flush=True)
        lines.append("| %s | %d | %.3f (%s) | %.3f (%s) | %.1f | %.1f |" % (name, args.rows, med["0"], ", ".join("%.3f" % v for v in q["res"]["0"]), med["1"],
                                                                          ", ".join("%.3f" % v for v in q["res"]["1"]), med["0"] / med["1"], row_ms))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
