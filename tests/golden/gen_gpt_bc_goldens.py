"""Golden vectors for policies.GPTBCPolicy: the reference's own Gpt_Agent.predict + GptPolicy + MinGPT (the BeT library's GPT with vocab_size = action_dim) + Scaler
(shim-imported, fixed-seed weights of trained-like magnitude) rolled out batch-1, environment by environment, TWICE - in f32 as shipped, and with model, scaling and
bounds in f64.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_gpt_bc_goldens.py
Output (committed): tests/golden/ref_gpt_bc_agent.npz - numeric arrays only; the file is written with fixed archive timestamps, so a second run reproduces it byte
for byte (``--check`` compares instead of writing).  Pins, against the actual reference code:
  * Gpt_Agent.predict            (agents/gpt_bc_agent.py:221-247): the deque of scaled observations grows to window_size and then slides
  * GptPolicy / MinGPT           (agents/gpt_bc_agent.py:23-75, agents/models/transformer/gpt_policy.py) with GPT (agents/models/bet/libraries/mingpt/model.py:128-250):
                                 ln_f and a bias-free head of action_dim rows
  * Scaler                       (agents/utils/scaler.py:10-113)
The agent is made without BaseAgent.__init__ (no datasets, no optimiser); min_action / max_action are built as Gpt_Agent.__init__ builds them.  There are no random
numbers.  D = max |f32 - f64| over the actions is the yardstick of tests/test_policies_gpt_bc.py.

What "f32 as shipped" is (printed by this script, restated by the policy): scale_input returns f32, the GPT runs in f32, ``actions.clamp_`` against the float64 bound
tensors keeps the f32 output (the comparison is made in f64: the same as clamping against the f32 roundings of the bounds), inverse_scale_output multiplies by the
float64 y_std and adds the float64 y_mean - the returned action is float64, an f64 product and sum on an f32 value.  For the f64 run the GPT is cast to f64 and
scale_input keeps f64.
"""
import importlib
import io
import os
import sys
import zipfile
from collections import deque

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims._StubFinder.ROOTS = ref_shims._StubFinder.ROOTS + ("hydra", "omegaconf", "tqdm", "torchsde", "torchdiffeq")
ref_shims.install()
import hydra  # noqa: E402  (stub)


def instantiate(cfg, *args, **kwargs):
    cfg = dict(cfg)
    target = cfg.pop("_target_")
    mod, name = target.rsplit(".", 1)
    cfg.update(kwargs)
    cfg.pop("_recursive_", None)
    return getattr(importlib.import_module(mod), name)(*args, **cfg)


hydra.utils.instantiate = instantiate

import agents.gpt_bc_agent as gpt_mod  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 6, 8
OBS, EMBD, LAYERS, HEADS, WINDOW, A = 20, 32, 2, 4, 5, 8


def make_scaler(seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, OBS)) * rng.uniform(0.05, 0.5, OBS) + rng.normal(size=OBS) * 0.3
    y = rng.normal(size=(400, A)) * 0.004 + rng.normal(size=A) * 0.002
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


def make_agent():
    torch.manual_seed(51)
    ag = object.__new__(gpt_mod.Gpt_Agent)
    ag.device = "cpu"
    ag.model = gpt_mod.GptPolicy(
        model=dict(_target_="agents.models.transformer.gpt_policy.MinGPT", discrete_input=False, input_dim=OBS, vocab_size=0, n_layer=LAYERS, n_head=HEADS, n_embd=EMBD,
                   device="cpu", block_size=WINDOW, action_dim=A),
        obs_encoder=dict(_target_="torch.nn.Identity", output_dim=OBS), visual_input=False, device="cpu")
    gpt = ag.model.model.model
    g = torch.Generator().manual_seed(52)
    with torch.no_grad():      # the initialisation (std 0.02, zero biases, unit LayerNorms) gives outputs near zero: values as after training
        for name, p in gpt.named_parameters():
            if name == "head.weight":
                p.copy_(torch.randn(p.shape, generator=g) * 0.45)      # outputs of a few units: some but not all reach the action clamp (the bounds sit near +-3)
            elif name == "pos_emb":
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif ".ln" in name or name.startswith("ln_f"):
                p.copy_((1.0 if name.endswith("weight") else 0.0) + torch.randn(p.shape, generator=g) * (0.2 if name.endswith("weight") else 0.1))
            elif name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.15)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    ag.scaler = make_scaler(53)
    ag.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to(ag.device)      # gpt_bc_agent.py:97-98
    ag.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to(ag.device)
    ag.window_size = WINDOW
    ag.obs_context = deque(maxlen=WINDOW)
    return ag


def run(ag, obs, f64):
    """The 48 predict calls; returns (actions [N, T, A], head outputs at the last token before the clamp [N, T, A], window lengths [N, T]) and the dtypes seen."""
    gpt = ag.model.model.model
    seen = []
    hook = gpt.head.register_forward_hook(lambda m, i, o: seen.append((i[0].detach().clone(), o.detach().clone())))
    keep = ag.scaler.scale_input
    if f64:
        ag.model.double()
        sc = ag.scaler
        sc.scale_input = lambda x: (x.double().to(sc.device) - sc.x_mean) / (sc.x_std + 1e-12)
    out = (np.zeros((N_ENV, T_STEPS, A)), np.zeros((N_ENV, T_STEPS, A)), np.zeros((N_ENV, T_STEPS), dtype=np.int64))
    try:
        for e in range(N_ENV):
            ag.reset()
            for t in range(T_STEPS):
                y = ag.predict(obs[e, t])
                xin, raw = seen[-1]
                assert raw.shape[0] == 1 and raw.shape[2] == A
                out[0][e, t] = np.asarray(y, dtype=np.float64).reshape(-1)
                out[1][e, t] = raw[0, -1].double().numpy()
                out[2][e, t] = raw.shape[1]
    finally:
        hook.remove()
        if f64:
            ag.scaler.scale_input = keep
            ag.model.float()
    return out, (xin.dtype, raw.dtype, np.asarray(y).dtype)


def npz_bytes(arrays: dict) -> bytes:
    """np.savez_compressed with fixed archive timestamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            one = io.BytesIO()
            np.lib.format.write_array(one, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            zf.writestr(info, one.getvalue(), compresslevel=9)
    return buf.getvalue()


def main():
    ag = make_agent()
    gpt = ag.model.model.model
    sd = {k: v.detach().clone() for k, v in gpt.state_dict().items()}
    lo, hi = ag.scaler.y_bounds[0].copy(), ag.scaler.y_bounds[1].copy()
    rng = np.random.default_rng(54)
    obs = (ag.scaler.x_mean.numpy() + rng.normal(size=(N_ENV, T_STEPS, OBS)) * ag.scaler.x_std.numpy()).astype(np.float32)
    r64, dt64 = run(ag, obs, True)
    r32, dt32 = run(ag, obs, False)
    assert all(torch.equal(sd[k], v) for k, v in gpt.state_dict().items()) and "head.bias" not in sd
    assert r64[2][0].tolist() == [min(t + 1, WINDOW) for t in range(T_STEPS)] and np.array_equal(r32[2], r64[2])      # the window grows, then slides
    D = float(np.abs(r32[0] - r64[0]).max())
    hit = (r64[1] < lo) | (r64[1] > hi)
    print("dtypes of (head input, head output, returned action): shipped run %s, f64 run %s; min_action %s, y_std %s" % (dt32, dt64, ag.min_action.dtype, ag.scaler.y_std.dtype))
    print("D = %.3e (largest |action - y_mean| %.3e); head outputs %.2f .. %.2f, bounds %s .. %s; outputs past a bound: %d of %d (f32 run: %d); window lengths %s"
          % (D, float(np.abs(r64[0] - ag.scaler.y_mean.numpy()).max()), r64[1].min(), r64[1].max(), np.round(lo, 2), np.round(hi, 2), int(hit.sum()), hit.size,
             int(((r32[1] < lo) | (r32[1] > hi)).sum()), r64[2][0].tolist()))
    assert 0 < hit.sum() < hit.size
    # clamping the f32 output against the f64 bounds equals clamping against their f32 roundings; the action is the f64 product and sum on that
    raw32 = r32[1].astype(np.float32)
    c32 = np.minimum(np.maximum(raw32, lo.astype(np.float32)), hi.astype(np.float32)).astype(np.float64)
    eps = np.float64(np.float32(1e-12))      # (the scaler adds 1e-12 * torch.ones(..): an f32 tensor)
    assert np.array_equal(c32 * (ag.scaler.y_std.numpy() + eps) + ag.scaler.y_mean.numpy(), r32[0])
    out = {"gb_sd__" + k.replace(".", "__"): v.numpy() for k, v in sd.items()}
    out.update(gb_cfg=np.array([OBS, EMBD, LAYERS, HEADS, WINDOW, A], dtype=np.int64), gb_obs=obs, gb_x_mean=ag.scaler.x_mean.numpy(), gb_x_std=ag.scaler.x_std.numpy(),
               gb_y_mean=ag.scaler.y_mean.numpy(), gb_y_std=ag.scaler.y_std.numpy(), gb_y_bounds=ag.scaler.y_bounds, gb_ref32=r32[0], gb_raw32=raw32, gb_ref64=r64[0],
               gb_raw64=r64[1], gb_D=np.array([D]))
    data = npz_bytes(out)
    dst = os.path.join(HERE, "ref_gpt_bc_agent.npz")
    if "--check" in sys.argv:
        same = open(dst, "rb").read() == data
        print("the committed file is reproduced byte for byte" if same else "the committed file DIFFERS from this run")
        sys.exit(0 if same else 1)
    with open(dst, "wb") as f:
        f.write(data)
    print("wrote", dst, "%.0f KB" % (len(data) / 1024))


if __name__ == "__main__":
    main()
