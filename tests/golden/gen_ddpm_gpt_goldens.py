"""Golden vectors for policies.DDPMGPTPolicy: the reference's own DiffusionAgent + Diffusion + DiffusionTransformerNetwork (shim-imported, fixed-seed weights of
trained-like magnitudes) rolled out batch-1, environment by environment.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_ddpm_gpt_goldens.py
Output (committed): tests/golden/ref_ddpm_gpt_agent.npz - numeric arrays only.  Pins, against the actual reference code:
  * DiffusionAgent.predict, window_size > 1     (agents/ddpm_agent.py:213-274)
  * Diffusion.sample / p_sample_loop / p_sample (agents/models/diffusion/gc_diffusion.py:117-216; cosine schedule, epsilon prediction, clip_denoised)
  * DiffusionTransformerNetwork                 (agents/models/diffusion/diffusion_models.py:409-667; linear_output, not goal conditioned)
  * Scaler                                      (agents/utils/scaler.py:10-113)
The agent is made without BaseAgent.__init__ (no datasets), as gen_agent_goldens.py makes its agents; use_ema is off.  torch.randn / torch.randn_like are patched for the
run to serve a banked normal per (environment, step, chain index, position, component): chain index T is the first iterate (p_sample_loop's randn), index i the noise
of reverse step i (index 0 is multiplied by the reference's nonzero mask).

The reference runs TWICE on the same bank: in f32 as shipped, and with the model, the schedule (every derived table computed again in f64 from the f32 betas, by policies.ddpm_schedule), the
scaling and the bank in f64.  Both action tables are stored; D = max |f32 - f64| is the reference's own f32 error on this problem - the yardstick of the replay tests.
The chain is continuous in its inputs (clamps, no discrete draw): no row needs to be left out of a comparison.
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

import agents.ddpm_agent as ddpm_mod  # noqa: E402
from agents.models.diffusion.gc_diffusion import Diffusion  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 6, 8
OBS, EMBD, LAYERS, HEADS, WINDOW, A, T = 20, 32, 2, 4, 5, 8, 8


def make_scaler(obs_dim, act_dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, obs_dim)) * rng.uniform(0.05, 0.5, obs_dim) + rng.normal(size=obs_dim) * 0.3
    y = rng.normal(size=(400, act_dim)) * 0.004
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


class NoiseBank:
    """Patches torch.randn / torch.randn_like: call c of a predict (c = 0: the first iterate, chain index T; c = 1 + j: reverse step T - 1 - j) returns
    bank[env, step, chain index, :L, :A] in the dtype of the run."""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.bank = torch.randn(N_ENV, T_STEPS, T + 1, WINDOW, A, generator=g)
        self.env = self.step = self.call = 0
        self.dtype = torch.float32

    def take(self, shape):
        shape = tuple(shape)
        assert len(shape) == 3 and shape[0] == 1 and shape[2] == A and self.call <= T
        k = T if self.call == 0 else T - self.call
        self.call += 1
        return self.bank[self.env, self.step, k, :shape[1]].reshape(shape).to(self.dtype).clone()

    def __enter__(self):
        self._r, self._rl = torch.randn, torch.randn_like
        torch.randn = lambda *s, **k: self.take(s[0] if len(s) == 1 and not isinstance(s[0], int) else s)
        torch.randn_like = lambda x, **k: self.take(x.shape)
        return self

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self._r, self._rl


def schedule_in_f64(d):
    """The reference's schedule attributes, filled with this project's own schedule code (policies.ddpm_schedule) run in f64 on the f32 betas."""
    from d3il_amd.policies import ddpm_schedule
    s = ddpm_schedule(d.betas.double())
    for ref_name, own in (("betas", "betas"), ("alphas", "alphas"), ("alphas_cumprod", "ac"), ("alphas_cumprod_prev", "ac_prev"), ("sqrt_recip_alphas_cumprod", "sqrt_recip_ac"),
                          ("sqrt_recipm1_alphas_cumprod", "sqrt_recipm1_ac"), ("posterior_variance", "post_var"), ("posterior_log_variance_clipped", "post_logvar"),
                          ("posterior_mean_coef1", "coef1"), ("posterior_mean_coef2", "coef2")):
        setattr(d, ref_name, s[own])


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
                assert bank.call == T + 1
    return ref


def main():
    torch.manual_seed(31)
    ag = object.__new__(ddpm_mod.DiffusionAgent)
    ag.device = "cpu"
    ag.model = Diffusion(state_dim=OBS, action_dim=A, beta_schedule="cosine", n_timesteps=T, loss_type="l2", clip_denoised=True, predict_epsilon=True, device="cpu",
                         model=dict(_target_="agents.models.diffusion.diffusion_models.DiffusionTransformerNetwork", state_dim=OBS, action_dim=A, device="cpu",
                                    goal_conditioned=False, embed_dim=EMBD, embed_pdrob=0.0, attn_pdrop=0.0, resid_pdrop=0.0, n_layers=LAYERS, n_heads=HEADS,
                                    goal_seq_len=0, obs_seq_len=WINDOW, linear_output=True))
    net = ag.model.model
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():      # the initialisation (std 0.02, zero biases, unit LayerNorms) makes the net nearly linear and its noise estimate tiny: values as after training
        for name, p in net.named_parameters():
            if name == "pos_emb":
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif name.startswith("action_pred"):
                p.copy_(torch.randn(p.shape, generator=g) * (0.25 if name.endswith("weight") else 0.1))      # a noise estimate of roughly unit size
            elif ".ln" in name or name.startswith("ln_f"):
                p.copy_((1.0 if name.endswith("weight") else 0.0) + torch.randn(p.shape, generator=g) * (0.2 if name.endswith("weight") else 0.1))
            elif name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.15)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    ag.scaler = make_scaler(OBS, A, 33)
    ag.model.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to("cpu")
    ag.model.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to("cpu")
    ag.window_size, ag.obs_context, ag.diffusion_kde, ag.use_ema = WINDOW, deque(maxlen=WINDOW), False, False
    obs = (np.random.default_rng(34).normal(size=(N_ENV, T_STEPS, OBS)) * 0.3).astype(np.float32).astype(np.float64)      # f32 values: predict() rounds its input to f32
    bank = NoiseBank(35)
    ref32 = rollout(ag, bank, obs)
    out = sd_arrays("dg_sd__", ag.model.state_dict())      # (f32, before the second run)
    # ---- the same run in f64: model, schedule, scaling, noise
    ag.model.double()
    schedule_in_f64(ag.model)
    sc = ag.scaler
    sc.scale_input = lambda x: (x.double() - sc.x_mean.double()) / (sc.x_std.double() + 1e-12)
    bank.dtype = torch.float64
    torch.set_default_dtype(torch.float64)      # SinusoidalPosEmb builds its frequencies in the default dtype
    ref64 = rollout(ag, bank, obs)
    torch.set_default_dtype(torch.float32)
    D = float(np.abs(ref32 - ref64).max())
    scaled = (ref64 - sc.y_mean.numpy()) / (sc.y_std.numpy() + 1e-12)
    lo, hi = sc.y_bounds[0], sc.y_bounds[1]
    inside = float(np.mean((scaled > lo + 1e-6) & (scaled < hi - 1e-6)))
    print("D = max |f32 - f64| of the reference: %.3e (actions of magnitude %.3e); action components strictly inside the bounds: %.2f" % (D, float(np.abs(ref64).max()), inside))
    assert 0.3 < inside < 1.0      # the clamp is exercised and is not all there is
    out.update(dg_cfg=np.array([OBS, EMBD, LAYERS, HEADS, WINDOW, A, T], dtype=np.int64), dg_obs=obs, dg_noise=bank.bank.numpy(), dg_ref32=ref32, dg_ref64=ref64,
               dg_D=np.array(D), dg_x_mean=sc.x_mean.numpy(), dg_x_std=sc.x_std.numpy(), dg_y_mean=sc.y_mean.numpy(), dg_y_std=sc.y_std.numpy(), dg_y_bounds=sc.y_bounds)
    dst = os.path.join(HERE, "ref_ddpm_gpt_agent.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, "%.0f KB" % (os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
