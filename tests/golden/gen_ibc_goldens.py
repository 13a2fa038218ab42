"""Golden vectors for policies.IBCPolicy: the reference's own IBCAgent + EBMMLP + LangevinMCMCSampler + Scaler (shim-imported, fixed-seed random weights) rolled
out batch-1, environment by environment, TWICE on the same banks of random numbers - in f32 as shipped, and with model, scaling, bounds and banks in f64.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_ibc_goldens.py
Output (committed): tests/golden/ref_ibc_agent.npz - numeric arrays only.  Pins, against the actual reference code:
  * IBCAgent.predict              (agents/ibc_agent.py:248-286), goal_conditioning False, no EMA
  * EBMMLP.forward                (agents/models/ibc/ebms.py:21-51) around ResidualMLPNetwork (agents/models/common/mlp.py:114-182)
  * LangevinMCMCSampler.infer     (agents/models/ibc/samplers/langevin_mcmc.py:129-163, 236-286) with PolynomialSchedule (schedulers.py:16-23)
  * Scaler                        (agents/utils/scaler.py:10-113)
The agent is made without BaseAgent.__init__ (no datasets).  Sampler settings: configs/agents/ibc_agent.yaml with the scripts' sampler_stepsize_init = 0.0493.
The three sources of randomness are patched to serve banks (f32 values, stored in the file): np.random.uniform -> the start points, torch.randn_like -> the
normals of every iteration, Categorical.sample -> the inverse-CDF rule of csrc/policy_ibc.h, pick = min(#{s : c_s <= u c_63}, 63), on the reference's own
probabilities in f64, driven by one banked u per (environment, step).  A banked u within EDGE = 1e-4 of an edge of the f64 run's normalised CDF is drawn again, so
every golden pick is decided and the replay tests leave no row out.  D = max |f32 - f64| over the actions (D_x: final samples, D_E: energies) is the yardstick of
tests/test_policies_ibc.py.

What "f32 as shipped" is: the sampler's bounds are a float64 array, so the first clamp promotes the samples to f64 and the chain's state, noise product and
update are f64 from then on, while ResidualMLPNetwork.forward casts every layer input to f32 - energies and gradients are f32.  For the f64 run that cast is taken out
(the layers are called in order, as forward does) and scale_input keeps f64.
"""
import importlib
import os
import sys

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

import agents.ibc_agent as ibc_mod  # noqa: E402
from agents.models.ibc.ebms import EBMMLP  # noqa: E402
from agents.models.ibc.samplers.langevin_mcmc import LangevinMCMCSampler  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 4, 4
OBS, A, HIDDEN, LAYERS, S, ITER = 6, 2, 128, 2, 64, 10
K = 2 * ITER
EDGE = 1e-4
SAMPLER = dict(noise_scale=0.1, noise_scale_infer=0.5, noise_shrink=0.894, train_samples=8, inference_samples=S, train_iterations=40, inference_iterations=ITER,
               sampler_stepsize_init=0.0493, sampler_stepsize_init_infer=0.5, second_inference_stepsize_init=0.00001, sampler_stepsize_decay=0.8,
               sampler_stepsize_final=0.00001, sampler_stepsize_power=2.0, use_polynomial_rate=True, second_inference_iteration=True, delta_action_clip=0.1, device="cpu")


def make_scaler(seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, OBS)) * rng.uniform(0.05, 0.5, OBS) + rng.normal(size=OBS) * 0.3
    y = rng.normal(size=(400, A)) * 0.004
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


def make_agent():
    ag = object.__new__(ibc_mod.IBCAgent)
    ag.device = "cpu"
    torch.manual_seed(21)
    ag.model = EBMMLP(mlp=dict(_target_="agents.models.common.mlp.ResidualMLPNetwork", input_dim=OBS + A, hidden_dim=HIDDEN, num_hidden_layers=LAYERS, output_dim=1, dropout=0,
                               activation="Mish", use_spectral_norm=False, use_norm=False, norm_style="BatchNorm", device="cpu"), device="cpu")
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():      # values as after training: an energy landscape with a few units of relief over the action box
        for name, p in ag.model.mlp.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * ((2.0 / p.shape[1]) ** 0.5 if name.endswith("weight") else 0.1))
    ag.sampler = LangevinMCMCSampler(**SAMPLER)
    ag.scaler = make_scaler(23)
    ag.set_bounds(ag.scaler)
    ag.goal_conditioning, ag.use_ema = False, False
    return ag


class Banks:
    """The three patches.  ``env`` / ``step`` say which row is running; ``decide`` (the f64 run) draws u again near an edge of the CDF."""

    def __init__(self, seed, lo, hi):
        rng = self.rng = np.random.default_rng(seed)
        self.x0 = (lo + rng.random((N_ENV, T_STEPS, S, A)) * (hi - lo)).astype(np.float32)
        self.x0 = np.minimum(np.maximum(self.x0, lo.astype(np.float32)), hi.astype(np.float32))      # f32 rounding must not leave the f64 box ...
        self.x0 = np.where(self.x0.astype(np.float64) < lo, np.nextafter(self.x0, np.float32(np.inf)), self.x0)
        self.x0 = np.where(self.x0.astype(np.float64) > hi, np.nextafter(self.x0, np.float32(-np.inf)), self.x0).astype(np.float32)
        self.noise = rng.normal(size=(N_ENV, T_STEPS, K, S, A)).astype(np.float32)
        self.u = (rng.integers(0, 1 << 24, size=(N_ENV, T_STEPS)) / float(1 << 24)).astype(np.float32)
        self.picks = np.zeros((N_ENV, T_STEPS), dtype=np.int64)
        self.cdf = np.zeros((N_ENV, T_STEPS, S))
        self.env = self.step = self.k = 0
        self.decide, self.redrawn = False, 0

    def uniform(self, low, high, size=None):
        assert tuple(size) == (S, A)
        return self.x0[self.env, self.step].astype(np.float64)

    def randn_like(self, t, **kw):
        z = torch.as_tensor(self.noise[self.env, self.step, self.k]).to(t.dtype).reshape(t.shape)
        self.k += 1
        return z

    def sample(self, cat, sample_shape=torch.Size()):
        c = np.cumsum(cat.probs.detach().double().numpy().reshape(S))
        e, t = self.env, self.step
        if self.decide:
            while np.abs(float(self.u[e, t]) * c[-1] - c).min() / c[-1] < EDGE:
                self.u[e, t] = np.float32(int(self.rng.integers(0, 1 << 24)) / float(1 << 24)); self.redrawn += 1
        self.cdf[e, t] = c / c[-1]
        self.picks[e, t] = min(int((c <= float(self.u[e, t]) * c[-1]).sum()), S - 1)
        return torch.tensor([self.picks[e, t]], dtype=torch.long)


def run(ag, banks, obs, f64):
    """The 16 predict calls; returns actions [N, T, A], final samples [N, T, S, A], energies [N, T, S], picks [N, T], all as f64 / i64 arrays."""
    seen = []
    hook = ag.model.register_forward_hook(lambda m, i, o: seen.append((i[1].detach().clone(), o.detach().clone())))
    keep = (np.random.uniform, torch.randn_like, torch.distributions.Categorical.sample, ag.scaler.scale_input, torch.get_default_dtype())
    np.random.uniform, torch.randn_like = banks.uniform, banks.randn_like
    torch.distributions.Categorical.sample = lambda self, sample_shape=torch.Size(): banks.sample(self, sample_shape)
    mlp = ag.model.mlp
    if f64:
        ag.model.double()
        torch.set_default_dtype(torch.float64)      # (compute_gradient's torch.ones for grad_outputs)
        sc = ag.scaler
        sc.scale_input = lambda x: (x.double() - sc.x_mean) / (sc.x_std + 1e-12)
        def forward(x):      # ResidualMLPNetwork.forward without its cast to f32
            for layer in mlp.layers:
                x = layer(x)
            return x
        mlp.forward = forward
    out = (np.zeros((N_ENV, T_STEPS, A)), np.zeros((N_ENV, T_STEPS, S, A)), np.zeros((N_ENV, T_STEPS, S)), np.zeros((N_ENV, T_STEPS), dtype=np.int64))
    try:
        for e in range(N_ENV):
            for t in range(T_STEPS):
                banks.env, banks.step, banks.k = e, t, 0
                out[0][e, t] = np.asarray(ag.predict(obs[e, t]), dtype=np.float64).reshape(-1)
                assert banks.k == K
                x, en = seen[-1]
                out[1][e, t], out[2][e, t], out[3][e, t] = x.double().numpy().reshape(S, A), en.double().numpy().reshape(S), banks.picks[e, t]
    finally:
        hook.remove()
        np.random.uniform, torch.randn_like, torch.distributions.Categorical.sample = keep[:3]
        torch.set_default_dtype(keep[4])
        if f64:
            ag.scaler.scale_input = keep[3]
            del mlp.forward
            ag.model.float()
    return out, (x.dtype, en.dtype)


def main():
    ag = make_agent()
    sd = {k: v.detach().clone() for k, v in ag.model.state_dict().items()}
    lo, hi = ag.scaler.y_bounds[0].copy(), ag.scaler.y_bounds[1].copy()
    banks = Banks(24, lo, hi)
    rng = np.random.default_rng(25)
    obs = (ag.scaler.x_mean.numpy() + rng.normal(size=(N_ENV, T_STEPS, OBS)) * ag.scaler.x_std.numpy()).astype(np.float32)
    banks.decide = True
    r64, dt64 = run(ag, banks, obs, True)
    banks.decide = False
    cdf64 = banks.cdf.copy()
    r32, dt32 = run(ag, banks, obs, False)
    assert all(torch.equal(sd[k], v) for k, v in ag.model.state_dict().items())
    D, Dx, DE = (float(np.abs(a - b).max()) for a, b in zip(r32[:3], r64[:3]))
    print("dtypes of (samples, energies): shipped run %s, f64 run %s" % (dt32, dt64))
    print("D = %.3e (actions %.3e), D_x = %.3e, D_E = %.3e, CDF difference %.3e, picks equal: %s, redrawn u: %d of %d, distinct picks %d" % (
        D, float(np.abs(r64[0]).max()), Dx, DE, float(np.abs(banks.cdf - cdf64).max()), np.array_equal(r32[3], r64[3]), banks.redrawn, N_ENV * T_STEPS, len(np.unique(r64[3]))))
    print("energy range %.2f .. %.2f; samples on a bound: %d of %d" % (r64[2].min(), r64[2].max(), int(((r64[1] <= lo) | (r64[1] >= hi)).sum()), r64[1].size))
    assert np.array_equal(r32[3], r64[3])
    smp = ag.sampler
    steps = [smp.sampler_stepsize_init_infer] + [smp.infer_schedule.get_rate(i) for i in range(1, ITER)] + [smp.second_inference_stepsize_init] * ITER
    other = LangevinMCMCSampler(**dict(SAMPLER, inference_iterations=7))      # the schedule object of another I
    steps7 = [other.sampler_stepsize_init_infer] + [other.infer_schedule.get_rate(i) for i in range(1, 7)] + [other.second_inference_stepsize_init] * 7
    out = {"ibc_sd__" + k.replace(".", "__"): v.numpy() for k, v in sd.items()}
    out.update(ibc_cfg=np.array([OBS, A, HIDDEN, LAYERS, S, ITER], dtype=np.int64), ibc_obs=obs, ibc_x0=banks.x0, ibc_noise=banks.noise, ibc_u=banks.u, ibc_steps=np.array(steps), ibc_steps7=np.array(steps7),
               ibc_settings=np.array([smp.noise_scale_infer, smp.delta_action_clip, smp.sampler_stepsize_init_infer, smp.sampler_stepsize_init, smp.sampler_stepsize_final,
                                      smp.sampler_stepsize_power, smp.second_inference_stepsize_init]),
               ibc_x_mean=ag.scaler.x_mean.numpy(), ibc_x_std=ag.scaler.x_std.numpy(), ibc_y_mean=ag.scaler.y_mean.numpy(), ibc_y_std=ag.scaler.y_std.numpy(), ibc_y_bounds=ag.scaler.y_bounds,
               ibc_ref32=r32[0], ibc_x32=r32[1].astype(np.float32), ibc_e32=r32[2].astype(np.float32), ibc_picks32=r32[3],
               ibc_ref64=r64[0], ibc_x64=r64[1], ibc_e64=r64[2], ibc_picks64=r64[3], ibc_cdf64=cdf64, ibc_D=np.array([D, Dx, DE]))
    dst = os.path.join(HERE, "ref_ibc_agent.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, "%.0f KB" % (os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
