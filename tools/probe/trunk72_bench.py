"""Timing of the 72-wide transformer trunk (n_embd 72, 4 heads, 4 layers) at 4096 lanes: the block chain alone, one
BESONativePolicy.predict_batch (16 sampling steps) and one DDPMGPTPolicy.predict_batch (8 timesteps), at window 1 (T = 3 tokens) and window 5 (T = 11).
Device events around 50 calls after 10 warm-up calls; one JSON line.

    python tools/probe/trunk72_bench.py [--tree DIR] [--label NAME] [--lanes 4096] [--calls 50] [--warmup 10]

--tree DIR imports d3il_amd from another checkout (the parent commit's, built there: it has no run_blocks and walks the chain block by block); the switch is the
environment's D3IL_POLICY_TRUNK72.  Alternate the trees in one visit, several runs each (profiles/trunk72/README.md)."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import torch
    from d3il_amd import policies as P
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / a.calls      # ms per call

    def chain(blocks, x, keep):
        if hasattr(P, "run_blocks"):
            return P.run_blocks(blocks, x, keep=keep)
        for blk in blocks[:-1]:
            x = blk(x)
        return blocks[-1](x, keep=keep)

    out = {"label": a.label, "lanes": a.lanes, "calls": a.calls, "switch": os.environ.get("D3IL_POLICY_TRUNK72"), "has_run_blocks": hasattr(P, "run_blocks"),
           "module": os.path.dirname(os.path.abspath(P.__file__))}
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for window in (1, 5):
            T = 2 * window + 1
            beso = P.BESONativePolicy.random(4, 2, device=dev, seed=1, embed_dim=72, n_layers=4, n_heads=4, window_size=window, num_sampling_steps=16, policy_seed=3)
            ddpm = P.DDPMGPTPolicy.random(4, 2, device=dev, seed=1, embed_dim=72, n_layers=4, n_heads=4, window_size=window, n_timesteps=8, policy_seed=3)
            x = torch.randn(a.lanes, T, 72, generator=g).to(dev)
            keep = torch.arange(2, T, 2, device=dev)
            obs = (torch.randn(a.lanes, 4, generator=g) * 0.5).to(dev)
            beso.ensure_packed()
            out["T%d_blocks_ms" % T] = timed(lambda: chain(beso.model.blocks, x, keep))
            out["T%d_beso_ms" % T] = timed(lambda: beso.predict_batch(obs))
            out["T%d_ddpm_gpt_ms" % T] = timed(lambda: ddpm.predict_batch(obs))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
