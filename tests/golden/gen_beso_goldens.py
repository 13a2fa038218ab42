"""Golden vectors for policies.BESONativePolicy: the reference's own BesoAgent + GCDenoiser + DiffusionGPT (shim-imported, fixed-seed weights of trained-like
magnitudes) rolled out batch-1, environment by environment.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_beso_goldens.py
Output (committed): tests/golden/ref_beso_agent.npz - numeric arrays only.  Pins, against the actual reference code:
  * BesoAgent.predict                           (agents/beso_agent.py:316-443; observation deque, action deque, final clamp)
  * sample_euler_ancestral / get_ancestral_step (k_diffusion/gc_sampling.py:107-114, 217-256) on get_sigmas_linear (41-44)
  * GCDenoiser                                  (k_diffusion/score_wrappers.py:18-99)
  * DiffusionGPT                                (k_diffusion/score_gpts.py:118-361; linear_output, not goal conditioned)
  * Scaler                                      (agents/utils/scaler.py:10-113)
The agent is made without BaseAgent.__init__ (no datasets), as gen_agent_goldens.py makes its agents; use_ema is off.  torch.randn / torch.randn_like are patched for the
run to serve a banked normal per (environment, step, draw, position, component): draw 0 is predict's randn for the newest action ([1, 1, A]: it sits at sequence
index 0 of the bank and goes to position L - 1 of the window), draw 1 + i the randn_like of sampling step i ([1, L, A], position by position).  The last sampling step
draws nothing (sigma_down = 0): S draws per predict.

The reference runs TWICE on the same bank: in f32 as shipped, and with the model, the sigma tables (the f32 schedule's values, every derived quantity in f64), the scaling
and the bank in f64.  Both action tables are stored; D = max |f32 - f64| is the reference's own f32 error on this problem - the yardstick of the replay tests.  The chain
is continuous in its inputs (one final clamp, no discrete draw): no row needs to be left out of a comparison.
"""
import importlib
import os
import sys
from collections import deque

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims._StubFinder.ROOTS = ref_shims._StubFinder.ROOTS + ("hydra", "omegaconf", "torchsde", "torchdiffeq")
ref_shims.install()
import hydra  # noqa: E402  (stub)


def instantiate(cfg, *args, **kwargs):
    cfg = dict(cfg)
    target = cfg.pop("_target_")
    cfg.pop("_recursive_", None)
    mod, name = target.rsplit(".", 1)
    cfg.update(kwargs)
    return getattr(importlib.import_module(mod), name)(*args, **cfg)


hydra.utils.instantiate = instantiate

import agents.beso_agent as beso_mod  # noqa: E402
from agents.models.beso.agents.diffusion_agents.k_diffusion.score_wrappers import GCDenoiser  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 6, 8
OBS, EMBD, LAYERS, HEADS, WINDOW, A, S = 20, 32, 2, 4, 5, 8, 16
SIGMA_MIN, SIGMA_MAX, SIGMA_DATA = 0.01, 1.0, 0.5


def make_scaler(obs_dim, act_dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, obs_dim)) * rng.uniform(0.05, 0.5, obs_dim) + rng.normal(size=obs_dim) * 0.3
    y = rng.normal(size=(400, act_dim)) * 0.004
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


class NoiseBank:
    """Patches torch.randn / torch.randn_like: call c of a predict (c = 0: the newest action's first iterate; c = 1 + i: sampling step i) returns
    bank[env, step, c, :L, :A] in the dtype of the run."""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.bank = torch.randn(N_ENV, T_STEPS, S, WINDOW, A, generator=g)
        self.env = self.step = self.call = 0
        self.dtype = torch.float32

    def take(self, shape):
        shape = tuple(shape)
        assert len(shape) == 3 and shape[0] == 1 and shape[2] == A and self.call < S and (self.call > 0 or shape[1] == 1)
        c = self.call
        self.call += 1
        return self.bank[self.env, self.step, c, :shape[1]].reshape(shape).to(self.dtype).clone()

    def __enter__(self):
        self._r, self._rl = torch.randn, torch.randn_like
        torch.randn = lambda *s, **k: self.take(s[0] if len(s) == 1 and not isinstance(s[0], int) else s)
        torch.randn_like = lambda x, **k: self.take(x.shape)
        return self

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self._r, self._rl


def sd_arrays(prefix, sd):
    return {prefix + k.replace(".", "__"): v.detach().cpu().numpy() for k, v in sd.items()}


def rollout(ag, bank, obs):
    ref = np.zeros((N_ENV, T_STEPS, A))
    with bank:
        for e in range(N_ENV):
            ag.reset()
            for t in range(T_STEPS):
                bank.env, bank.step, bank.call = e, t, 0
                ref[e, t] = np.asarray(ag.predict(obs[e, t])).reshape(-1)
                assert bank.call == S
    return ref


def main():
    torch.manual_seed(41)
    ag = object.__new__(beso_mod.BesoAgent)
    ag.device = "cpu"
    ag.model = GCDenoiser(sigma_data=SIGMA_DATA, inner_model=dict(
        _target_="agents.models.beso.agents.diffusion_agents.k_diffusion.score_gpts.DiffusionGPT", state_dim=OBS, action_dim=A, goal_conditioned=False, embed_dim=EMBD,
        embed_pdrob=0, attn_pdrop=0.0, resid_pdrop=0.0, n_layers=LAYERS, n_heads=HEADS, goal_seq_len=1, obs_seq_len=WINDOW, sigma_vocab_size=8, device="cpu",
        linear_output=True, time_embedding_fn=None))
    net = ag.model.inner_model
    g = torch.Generator().manual_seed(42)
    with torch.no_grad():      # the initialisation (std 0.02, zero biases, unit LayerNorms) makes the net nearly linear and its output tiny: values as after training
        for name, p in net.named_parameters():
            if name == "pos_emb":
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif name.startswith("action_pred"):
                p.copy_(torch.randn(p.shape, generator=g) * (0.25 if name.endswith("weight") else 0.1))      # an output of roughly unit size
            elif ".ln" in name or name.startswith("ln_f"):
                p.copy_((1.0 if name.endswith("weight") else 0.0) + torch.randn(p.shape, generator=g) * (0.2 if name.endswith("weight") else 0.1))
            elif name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.15)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    ag.scaler = make_scaler(OBS, A, 43)
    ag.model.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to("cpu")
    ag.model.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to("cpu")
    ag.window_size, ag.obs_context, ag.action_context = WINDOW, deque(maxlen=WINDOW), deque(maxlen=WINDOW - 1)
    ag.sampler_type, ag.num_sampling_steps, ag.sigma_min, ag.sigma_max, ag.sigma_data, ag.rho = "euler_ancestral", S, SIGMA_MIN, SIGMA_MAX, SIGMA_DATA, 5
    ag.noise_scheduler, ag.use_ema = "linear", False
    obs = (np.random.default_rng(44).normal(size=(N_ENV, T_STEPS, OBS)) * 0.3).astype(np.float32).astype(np.float64)      # f32 values: predict() rounds its input to f32
    bank = NoiseBank(45)
    ref32 = rollout(ag, bank, obs)
    out = sd_arrays("bs_sd__", ag.model.state_dict())      # (f32, before the second run)
    sig32 = ag.get_noise_schedule(S, "linear").clone()
    # ---- the same run in f64: model, sigma tables (the f32 schedule's values), scaling, noise
    ag.model.double()
    net.sigma_emb.register_forward_pre_hook(lambda mod, inp: (inp[0].double(),))      # (the reference hands sigma_emb log(sigma) / 4 rounded to f32: that rounding stays)
    ag.get_noise_schedule = lambda n, kind: sig32.double()
    sc = ag.scaler
    sc.scale_input = lambda x: (x.double() - sc.x_mean.double()) / (sc.x_std.double() + 1e-12)
    bank.dtype = torch.float64
    torch.set_default_dtype(torch.float64)
    ref64 = rollout(ag, bank, obs)
    torch.set_default_dtype(torch.float32)
    D = float(np.abs(ref32 - ref64).max())
    scaled = (ref64 - sc.y_mean.numpy()) / (sc.y_std.numpy() + 1e-12)
    lo, hi = sc.y_bounds[0], sc.y_bounds[1]
    inside = float(np.mean((scaled > lo + 1e-6) & (scaled < hi - 1e-6)))
    print("D = max |f32 - f64| of the reference: %.3e (actions of magnitude %.3e); action components strictly inside the bounds: %.2f" % (D, float(np.abs(ref64).max()), inside))
    assert 0.05 < inside      # the clamp is not all there is
    out.update(bs_cfg=np.array([OBS, EMBD, LAYERS, HEADS, WINDOW, A, S], dtype=np.int64), bs_sigma=np.array([SIGMA_MIN, SIGMA_MAX, SIGMA_DATA]), bs_obs=obs,
               bs_noise=bank.bank.numpy(), bs_ref32=ref32, bs_ref64=ref64, bs_D=np.array(D), bs_x_mean=sc.x_mean.numpy(), bs_x_std=sc.x_std.numpy(),
               bs_y_mean=sc.y_mean.numpy(), bs_y_std=sc.y_std.numpy(), bs_y_bounds=sc.y_bounds)
    dst = os.path.join(HERE, "ref_beso_agent.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, "%.0f KB" % (os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
