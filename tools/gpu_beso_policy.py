"""Measurement of the native BESO policy (policies.BESONativePolicy): 120 wide / 6 layers / 6 heads, window 5, 16 sampling steps, sigma 0.01 .. 1, on
Stacking observations (obs 20 -> 8).

  python tools/gpu_beso_policy.py [--rows 4096] [--calls 20] [--runs 3] [--out FILE.md]

``predict_batch`` ms at ``rows`` environments with a full window, alternating a / b / c / d / a / .. in ONE process (``runs`` runs of ``calls`` calls each, event pair
around a run, median of the runs), for
  (a) BESOPolicy(use_graph=True) as bench.py builds it - the parent's path: torch.randn on the device generator, its own captured sampling loop;
  (b) BESONativePolicy with the torch glue (D3IL_POLICY_BESO_STEP=0; its normals come from torch.randn on the device through ``noise_in`` - the host Philox of the
      fallback would only add a host round trip per draw that the glue itself does not need);
  (c) BESONativePolicy with the step kernel (Philox inside the kernel), eager;
  (d) the same under CapturedPolicy: one graph replay per call.
Then one sampling step's glue alone - the step kernel and the torch ops of one step index on one state (event pair around back-to-back calls).
Prints one JSON line and a markdown table (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3il_amd import policies as P  # noqa: E402


def timed_calls(pol, obs, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        pol.predict_batch(obs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def chain_state(pol, obs):
    """The state dict of one chain (as predict_batch builds it) plus hidden rows, for timing one step index alone."""
    n, dev, m = obs.shape[0], obs.device, pol.model
    pol.ensure_packed()
    pol._state(n)
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
    import bench
    os.environ.pop("D3IL_POLICY_GRAPH", None)
    parent = bench._random_beso(dev)      # (a): exactly what bench.py --policy beso runs
    assert parent.use_graph
    A, obs_dim = 8, 20
    kern = P.BESONativePolicy.random(obs_dim, A, device=dev, seed=1)
    mk = lambda **kw: P.BESONativePolicy(kern.model, kern.scaler, kern.W, kern.S, kern.sigma_min, kern.sigma_max, sigma_data=kern.sigma_data, **kw)
    glue = mk(noise_in=lambda d, n, W=kern.W: torch.randn(n, W, A, device=dev))
    cap = P.CapturedPolicy(mk())
    pols = {"a": (parent, None), "b": (glue, "0"), "c": (kern, "1"), "d": (cap, "1")}
    obs = torch.randn(args.rows, obs_dim, device=dev) * 0.5

    def run(key, calls):
        pol, mode = pols[key]
        if mode is None:
            os.environ.pop("D3IL_POLICY_BESO_STEP", None)
        else:
            os.environ["D3IL_POLICY_BESO_STEP"] = mode
        return timed_calls(pol, obs, calls)

    for key in pols:      # warm-up of all forms, windows filled, graphs captured
        run(key, 7)
    res = {key: [] for key in pols}
    for _ in range(args.runs):
        for key in pols:
            res[key].append(run(key, args.calls))
    os.environ.pop("D3IL_POLICY_BESO_STEP", None)
    # one step index alone, on one state
    alone = {}
    for name, pol in (("kernel", kern), ("torch", glue)):
        st, hk = chain_state(pol, obs)
        fn = pol._step_kernel if name == "kernel" else pol._step_torch
        reps = 200 if name == "kernel" else 50
        for _ in range(5):
            fn(st, 7, hk)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(st, 7, hk)
        e1.record()
        torch.cuda.synchronize()
        alone[name] = e0.elapsed_time(e1) / reps * 1e3
    med = {key: statistics.median(v) for key, v in res.items()}
    out = {"rows": args.rows, "calls": args.calls, "besopolicy_graph_ms": res["a"], "native_torch_glue_ms": res["b"], "native_kernel_eager_ms": res["c"],
           "native_kernel_captured_ms": res["d"], "median_ms": med, "step_kernel_alone_us": alone["kernel"], "torch_glue_alone_us": alone["torch"]}
    print(json.dumps(out), flush=True)
    fmt = lambda key: "%.3f (%s)" % (med[key], ", ".join("%.3f" % v for v in res[key]))
    lines = ["| rows | (a) BESOPolicy, own graph (ms) | (b) native, torch glue (ms) | (c) native, step kernel, eager (ms) | (d) native, step kernel, CapturedPolicy (ms) | "
             "step kernel alone (us / step) | torch glue alone (us / step) |", "|---|---|---|---|---|---|---|",
             "| %d | %s | %s | %s | %s | %.1f | %.1f |" % (args.rows, fmt("a"), fmt("b"), fmt("c"), fmt("d"), alone["kernel"], alone["torch"])]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
