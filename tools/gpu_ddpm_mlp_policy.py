"""Measurement of the batched DDPM-MLP policy on the Philox stream (policies.DDPMNativePolicy) at the seven DDPM-MLP shapes the reference
configures (scripts/*/ddpm_benchmark.sh with configs/*_config.yaml).

  python tools/gpu_ddpm_mlp_policy.py [--rows 4096] [--calls 20] [--runs 5] [--out profiles/ddpm_mlp/README.md]

Per shape, ``predict_batch`` ms at ``rows`` environments for (b) the torch path (D3IL_POLICY_DDPM_MLP_CHAIN=0; the normals are a device ``torch.randn`` handed in
through ``noise_in`` - the host Philox of the fallback would add a synchronisation and NumPy work per call that the layers themselves do not need), (c) the chain
kernel called eagerly (Philox inside) and (d) the chain kernel under CapturedPolicy, alternating b / c / d in one process (``runs`` runs of ``calls`` calls each, an
event pair around a run, median and range of the runs); and (a) the agents.RowwiseAgent path - one batch-1 predict per environment and step on torch's layers with
device ``torch.randn`` draws, a host-to-device and a device-to-host copy, what ``as_batched`` gave a DDPM-MLP agent before this policy - on 64 environments.  At the
Sorting-4 shape, the only one it is built for, the older policies.DDPMPolicy (k_ddpm_mlp_f32, its ``torch.randn`` of the (T + 1) x rows x 2 normals inside the timed
region) runs in the same alternation.  Prints one JSON line per shape and writes the markdown table to --out."""
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

SWITCH = "D3IL_POLICY_DDPM_MLP_CHAIN"
#          name        obs  A  t_dim  T  hidden  hidden layers
SHAPES = (("avoiding", 4, 2, 24, 4, 128, 6), ("pushing", 10, 2, 16, 8, 128, 6), ("sorting-2", 10, 2, 4, 4, 128, 6), ("sorting-4", 16, 2, 8, 4, 256, 8),
          ("sorting-6", 22, 2, 4, 4, 256, 8), ("aligning", 20, 3, 8, 24, 128, 6), ("stacking", 20, 8, 4, 4, 256, 8))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


class Batch1Agent:
    """DiffusionAgent.predict on one environment as the reference computes it: numpy row in, the reverse chain on a [1, obs] row with torch's own layers and device
    torch.randn draws (T + 1 of them), clamp, inverse scaling, numpy [1, A] out."""

    def __init__(self, pol):
        self.pol = pol

    @torch.no_grad()
    def predict(self, row):
        p = self.pol
        s = p.scaler.scale_input(torch.from_numpy(row).float().to(p.device).unsqueeze(0))
        x = torch.randn(1, p.A, device=p.device)
        for i in reversed(range(p.T)):
            eps = p.model(x, torch.full((1,), i, device=p.device, dtype=torch.long), s)
            sc = p._sched[i]
            x0 = (sc[0] * x - sc[1] * eps).clamp(p.lo, p.hi)
            x = sc[2] * x0 + sc[3] * x + sc[4] * torch.randn_like(x)
        return (x.clamp(p.lo, p.hi) * p.out_scale + p.out_shift).detach().cpu().numpy()

    def reset(self):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ddpm_mlp", "README.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    os.environ.pop(SWITCH, None)
    cases = {}
    for name, obs_dim, A, td, T, hidden, nh in SHAPES:
        mk = lambda **kw: P.DDPMNativePolicy.random(obs_dim, A, device=dev, seed=1, hidden_dim=hidden, n_blocks=nh // 2, t_dim=td, n_timesteps=T, **kw)
        kern, inner = mk(), mk()
        layers = mk(noise_in=lambda k, n, A=A: torch.randn(n, A, device=dev))
        cap = inner.captured()
        obs = torch.randn(args.rows, obs_dim, device=dev) * 0.5
        assert kern._kernel_shape(), name
        forms = {"torch": (lambda p=layers, o=obs: p.predict_batch(o), "0"), "kernel": (lambda p=kern, o=obs: p.predict_batch(o), "1"),
                 "captured": (lambda p=cap, o=obs: p.predict_batch(o), "1")}
        if name == "sorting-4":
            old = P.DDPMPolicy(kern.model, kern.scaler, T)
            assert old.fused_ok()
            forms["parent"] = (lambda p=old, o=obs: p.predict_batch(o), "1")
        cases[name] = {"forms": forms, "pol": kern, "obs": obs, "res": {k: [] for k in forms}}
    for q in cases.values():      # warm-up of every form (the capture among them)
        for form, (fn, mode) in q["forms"].items():
            os.environ[SWITCH] = mode
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    for _ in range(args.runs):      # the shapes and the forms alternate in one process
        for q in cases.values():
            for form, (fn, mode) in q["forms"].items():
                os.environ[SWITCH] = mode
                q["res"][form].append(timed(fn, args.calls))
    os.environ.pop(SWITCH, None)
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
    lines = ["# DDPM-MLP on the Philox stream: `predict_batch` at %d environments" % args.rows, "",
             "Written by `tools/gpu_ddpm_mlp_policy.py --rows %d --calls %d --runs %d` on one MI355X: per form the median of %d runs of %d calls each, the range of the runs "
             "in brackets (the run-to-run spread), all forms and shapes alternating in one process after a warm-up.  (a) is the row-by-row adapter on 64 environments, "
             "wall clock per step." % (args.rows, args.calls, args.runs, args.runs, args.calls), "",
             "| shape (obs, A, t_dim, T, hidden / hidden layers) | (b) torch path (ms) | (c) kernel, eager (ms) | (d) kernel, captured (ms) | b / c | (a) RowwiseAgent, 64 envs (ms / step) |",
             "|---|---|---|---|---|---|"]
    parent_line = None
    os.environ["D3IL_POLICY_FUSED_RESMLP"] = "0"      # the row-by-row adapter runs torch's own layers, as the reference agent does
    for (name, obs_dim, A, td, T, hidden, nh), q in zip(SHAPES, cases.values()):
        rw = RowwiseAgent(Batch1Agent(q["pol"]), 64)
        o64 = q["obs"][:64]
        rw.predict_batch(o64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            rw.predict_batch(o64)
        torch.cuda.synchronize()
        row_ms = (time.perf_counter() - t0) / 2 * 1e3
        res = q["res"]
        med = {k: statistics.median(v) for k, v in res.items()}
        print(json.dumps({"shape": name, "rows": args.rows, **{k + "_ms": v for k, v in res.items()}, **{k + "_ms_median": v for k, v in med.items()},
                          "rowwise_64_envs_ms_per_step": row_ms}), flush=True)
        lines.append("| %s (%d, %d, %d, %d, %d / %d) | %s | %s | %s | %.1f | %.1f |" % (name, obs_dim, A, td, T, hidden, nh, fmt(res["torch"]), fmt(res["kernel"]), fmt(res["captured"]),
                                                                                    med["torch"] / med["kernel"], row_ms))
        if "parent" in res:
            spread = max(max(res[k]) - min(res[k]) for k in ("kernel", "parent"))
            parent_line = ("Sorting-4, the shape the older `DDPMPolicy` (`k_ddpm_mlp_f32`, `torch.randn` of its (T + 1) x rows x 2 normals inside the timed region) is built "
                           "for, in the same alternation: parent %s ms, new kernel eager %s ms, captured %s ms; new eager - parent = %+.3f ms against a run-to-run spread "
                           "of %.3f ms (the larger range of the two)." % (fmt(res["parent"]), fmt(res["kernel"]), fmt(res["captured"]), med["kernel"] - med["parent"], spread))
    os.environ.pop("D3IL_POLICY_FUSED_RESMLP", None)
    lines += ["", parent_line]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
