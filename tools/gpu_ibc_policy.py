"""Measurement of the batched IBC policy (policies.IBCPolicy): hidden 128 / 3 blocks on Avoiding-like observations (obs 4 -> 2) and hidden 256 /
4 blocks on Stacking-like ones (obs 20 -> 8), 64 samples, 10 + 10 Langevin iterations.

  python tools/gpu_ibc_policy.py [--rows 4096] [--calls 20] [--runs 3] [--out FILE.md]

Per shape: ``predict_batch`` ms at ``rows`` environments for (a) the torch-op chain (D3IL_POLICY_IBC_FUSED=0; its random numbers come from torch on the device through
``x0_in`` / ``noise_in`` / ``u_in`` - the host Philox of the fallback would add seconds of NumPy per call that the chain itself does not need) and (b) the kernel
(Philox inside), alternating a / b / a / b .. in one process (``runs`` runs of ``calls`` calls each, event pair around a run, median of the runs); the achieved share
of the f32 matrix-core peak (157.3 TFLOP/s) from the multiply-adds of the layers; and one line for the agents.RowwiseAgent path - one batch-1 predict per environment and
step, each K torch.autograd.grad passes and one forward pass on 64 samples with a host round trip, what an IBCAgent got before this policy - on 64 environments.
Prints one JSON line per figure and a markdown table (also written to --out)."""
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

PEAK_F32_MATRIX = 157.3e12


def timed_calls(pol, obs, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        pol.predict_batch(obs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def flops_per_env_step(pol):
    """Multiply-adds x 2 of the layers: K evaluations forward + backward and one forward, on S samples."""
    lin_in, blocks, _ = pol.model._parts()
    H, nb = lin_in.out_features, len(blocks)
    fwd = 2 * (lin_in.in_features * H + 2 * nb * H * H + H)
    bwd = 2 * (2 * nb * H * H + pol.A * H)
    return pol.S * (pol.K * (fwd + bwd) + fwd)


class AutogradBatch1Agent:
    """IBCAgent.predict on one environment as the reference computes it: numpy row in, K torch.autograd.grad passes through torch's own layers, numpy [1, A] out."""

    def __init__(self, pol):
        self.pol = pol

    def energy(self, rows):
        F = torch.nn.functional
        lin_in, blocks, lin_out = self.pol.model._parts()
        x = lin_in(rows)
        for l1, l2 in blocks:
            x = x + l2(F.mish(l1(F.mish(x))))
        return lin_out(x)[:, 0]

    def predict(self, row):
        p = self.pol
        s = p.scaler.scale_input(torch.as_tensor(row, dtype=torch.float32, device=p.device).reshape(1, -1)).expand(p.S, -1)
        x = p.lo + torch.rand(p.S, p.A, device=p.device) * (p.hi - p.lo)
        for k in range(p.K):
            with torch.enable_grad():
                xa = x.detach().requires_grad_(True)
                g, = torch.autograd.grad(self.energy(torch.cat([s, xa], dim=1)).sum(), xa)
            d = torch.minimum(torch.maximum(p.coef[k, 0] * g + p.coef[k, 1] * (torch.randn_like(x) * p.noise_scale), -p.clip), p.clip)
            x = torch.minimum(torch.maximum(x - d, p.lo), p.hi)
        with torch.no_grad():
            e = self.energy(torch.cat([s, x], dim=1))
        pick = torch.distributions.Categorical(torch.softmax(-e, dim=0)).sample()
        return (x[pick] * p.out_scale + p.out_shift).reshape(1, -1).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["| shape | rows | predict_batch, torch chain (ms) | predict_batch, kernel (ms) | kernel: TFLOP/s (share of the f32 matrix peak) | RowwiseAgent, 64 envs (ms / step) |",
             "|---|---|---|---|---|---|"]
    shapes = (("hidden 128 / 3 blocks, obs 4 -> 2", 4, 2, 128, 3), ("hidden 256 / 4 blocks, obs 20 -> 8", 20, 8, 256, 4))
    pols = {}
    for name, obs_dim, A, hidden, nb in shapes:
        kern = P.IBCPolicy.random(obs_dim, A, device=dev, seed=1, hidden_dim=hidden, n_blocks=nb)
        S, K = kern.S, kern.K
        chain = P.IBCPolicy(kern.model, kern.scaler, kern.steps, noise_scale=kern.noise_scale, delta_action_clip=kern.delta_action_clip,
                            x0_in=lambda n, A=A, S=S, k=kern: k.lo + torch.rand(n, S, A, device=dev) * (k.hi - k.lo), noise_in=lambda n, A=A, S=S, K=K: torch.randn(K, n, S, A, device=dev),
                            u_in=lambda n: torch.rand(n, device=dev))
        pols[name] = {"0": chain, "1": kern, "obs": torch.randn(args.rows, obs_dim, device=dev) * 0.5, "res": {"0": [], "1": []}}
    for name in pols:      # warm-up of both forms
        for mode in ("0", "1"):
            os.environ["D3IL_POLICY_IBC_FUSED"] = mode
            for _ in range(2):
                pols[name][mode].predict_batch(pols[name]["obs"])
    torch.cuda.synchronize()
    for _ in range(args.runs):      # the two shapes and the two forms alternate in one process
        for name in pols:
            for mode in ("0", "1"):
                os.environ["D3IL_POLICY_IBC_FUSED"] = mode
                pols[name]["res"][mode].append(timed_calls(pols[name][mode], pols[name]["obs"], args.calls))
    os.environ.pop("D3IL_POLICY_IBC_FUSED", None)
    for name, obs_dim, A, hidden, nb in shapes:
        q = pols[name]
        rw = RowwiseAgent(AutogradBatch1Agent(q["1"]), 64)
        o64 = q["obs"][:64]
        rw.predict_batch(o64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        row_ms = (time.perf_counter() - t0) / 2 * 1e3
        med = {m: statistics.median(q["res"][m]) for m in ("0", "1")}
        tflops = flops_per_env_step(q["1"]) * args.rows / (med["1"] * 1e-3) / 1e12
        out = {"shape": name, "rows": args.rows, "torch_chain_ms": q["res"]["0"], "kernel_ms": q["res"]["1"], "torch_chain_ms_median": med["0"], "kernel_ms_median": med["1"],
               "gflop_per_env_step": flops_per_env_step(q["1"]) / 1e9, "kernel_tflops": tflops, "share_of_f32_matrix_peak": tflops * 1e12 / PEAK_F32_MATRIX, "rowwise_64_envs_ms_per_step": row_ms}
        print(json.dumps(out), flush=True)
        lines.append("| %s | %d | %.2f (%s) | %.2f (%s) | %.1f (%.1f %%) | %.0f |" % (name, args.rows, med["0"], ", ".join("%.2f" % v for v in q["res"]["0"]), med["1"],
                                                                                    ", ".join("%.2f" % v for v in q["res"]["1"]), tflops, 100 * tflops * 1e12 / PEAK_F32_MATRIX, row_ms))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
