"""Golden vectors for policies.DDPMNativePolicy: the reference's own DiffusionAgent + Diffusion + DiffusionMLPNetwork + Scaler (shim-imported, fixed-seed weights of
trained-like magnitudes) rolled out batch-1, environment by environment, in three cases.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_ddpm_mlp_goldens.py
Output (committed): tests/golden/ref_ddpm_mlp_agent.npz - numeric arrays only.  Pins, against the actual reference code:
  * DiffusionAgent.predict, window_size 1 and 5  (agents/ddpm_agent.py:213-274)
  * Diffusion.sample / p_sample_loop / p_sample  (agents/models/diffusion/gc_diffusion.py:101-216; cosine schedule, epsilon prediction, clip_denoised)
  * DiffusionMLPNetwork                          (agents/models/diffusion/diffusion_models.py:20-118; residual style, Mish, not goal conditioned)
  * ResidualMLPNetwork                           (agents/models/common/mlp.py:114-182)
  * Scaler                                       (agents/utils/scaler.py:10-113)
Cases (6 environments x 8 steps each):
  a  avoiding shape  A 2, t_dim 24, obs  4, T  4, window 1, hidden 128 / 2 hidden layers   a shape of the chain kernel
  b  aligning shape  A 3, t_dim  8, obs 20, T 24, window 1, hidden  32 / 4                 the torch path
  c  stacking shape  A 8, t_dim  4, obs 20, T  4, window 5, hidden  32 / 4                 the window claim: the policy keeps no history
The agent is made without BaseAgent.__init__ (no datasets), as gen_ddpm_gpt_goldens.py makes its agent; use_ema is off.  torch.randn / torch.randn_like are patched
for the run to serve a banked normal per (environment, step, call, position, component): call 0 is the first iterate (p_sample_loop's randn), call 1 + j the noise of
reverse step T - 1 - j.  The reference makes T + 1 calls per predict; the last one (step 0) is multiplied by its nonzero mask and thrown away, so calls 0 .. T - 1 are
the policy's draws k.  At window L the reference draws [1, L, A]: the bank serves its LAST L positions, so the newest position - the only one predict returns - is
always bank[.., W - 1, :], which is the policy's draw.

Case c needs one repair of the reference: DiffusionMLPNetwork.forward reshapes the time embedding to [batch, 1, t_dim] and concatenates it with the [batch, L, .] window
along the last axis (diffusion_models.py:95-104), which torch.cat refuses for L >= 2 - as shipped, this denoiser runs at window 1 (what every ddpm_benchmark.sh
configures) and on the first step of an episode only.  The generator asserts that, and then runs case c with the time embedding broadcast over the L positions
(``expand``) - the only reading under which the shipped line runs, and what policies.DiffusionMLP.forward has always done; everything else (the sampler over
[1, L, A], the layers, the position predict returns) is the reference's own code.

The reference runs TWICE on the same bank: in f32 as shipped, and with the model, the schedule (every derived table computed again in f64 from the f32 betas, by
policies.ddpm_schedule), the scaling and the bank in f64 (ResidualMLPNetwork.forward's cast to f32 taken out: the layers are called in order, as forward does).  Both
action tables are stored; D = max |f32 - f64| per case is the reference's own f32 error on this problem - the yardstick of the replay tests.  The chain is continuous
in its inputs (clamps, no discrete draw): no row needs to be left out of a comparison.

D has to be a yardstick, not a lottery.  At the first reverse step x0 = sra x - srm1 eps with sra and srm1 of 20 .. 30: against bounds of +-3 (the range of plain
normal action data) nearly every row is clipped there, the few that escape carry the f32 error of their eps times srm1, and D is the maximum over a handful of the 96
.. 384 values - it moved by a factor of seven (6.2e-8 -> 8.7e-9 in case a) when nothing but the gain of the output layer changed.  With the bounds the outliers give, a
good share of the rows escape the first clip and D is the maximum over a population; the generator asserts that at least eight values deviate by more than D / 4
(with the narrow bounds it was one or two).
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
from agents.models.common.mlp import ResidualMLPNetwork  # noqa: E402
from agents.models.diffusion.gc_diffusion import Diffusion  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 6, 8
#        name  obs  A  t_dim  T  window  hidden  hidden layers  seed
CASES = (("a", 4, 2, 24, 4, 1, 128, 2, 100),
         ("b", 20, 3, 8, 24, 1, 32, 4, 200),
         ("c", 20, 8, 4, 4, 5, 32, 4, 300))


def make_scaler(obs_dim, act_dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, obs_dim)) * rng.uniform(0.05, 0.5, obs_dim) + rng.normal(size=obs_dim) * 0.3
    y = rng.normal(size=(400, act_dim)) * 0.004
    y[0], y[1] = 0.04, -0.04      # two outliers, ten standard deviations out, set the bounds (y_bounds = the data's range): about +-8.5 in scaled space - see D below
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


class NoiseBank:
    """Patches torch.randn / torch.randn_like: call c of a predict returns bank[env, step, c, W - L :, :A] (L = the window length of the call) in the dtype of the run."""

    def __init__(self, seed, T, W, A):
        g = torch.Generator().manual_seed(seed)
        self.bank = torch.randn(N_ENV, T_STEPS, T + 1, W, A, generator=g)
        self.T, self.W, self.A = T, W, A
        self.env = self.step = self.call = 0
        self.dtype = torch.float32

    def take(self, shape):
        shape = tuple(shape)
        assert shape[0] == 1 and shape[-1] == self.A and len(shape) in (2, 3) and self.call <= self.T
        L = shape[1] if len(shape) == 3 else 1
        out = self.bank[self.env, self.step, self.call, self.W - L:].reshape(shape).to(self.dtype).clone()
        self.call += 1
        return out

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


def rollout(ag, bank, obs, x0_log):
    ref = np.zeros((N_ENV, T_STEPS, bank.A))
    inner = ag.model.predict_start_from_noise

    def logged(x_t, t, noise):      # the x0 prediction in front of its clamp: the newest position only
        out = inner(x_t, t, noise)
        x0_log.append(out.detach().double().reshape(-1, bank.A)[-1].numpy().copy())
        return out

    ag.model.predict_start_from_noise = logged
    with bank:
        for e in range(N_ENV):
            ag.reset()
            for t in range(T_STEPS):
                bank.env, bank.step, bank.call = e, t, 0
                ref[e, t] = np.asarray(ag.predict(obs[e, t])).reshape(-1)
                assert bank.call == bank.T + 1
    del ag.model.predict_start_from_noise
    return ref


def forward_without_cast(self, x):      # ResidualMLPNetwork.forward (mlp.py:169-182) without x.to(torch.float32)
    for layer in self.layers:
        x = layer(x)
    return x


def broadcast_time(net):
    """The repair of case c (module docstring): forward with the time embedding expanded over the window positions where the window is longer than one."""
    shipped = net.forward

    def forward(x, t, state, goal):
        if state.dim() == 3 and state.shape[1] > 1:
            emb = net.temp_layers(t)[:, None, :].expand(-1, state.shape[1], -1)
            return net.layers(torch.cat([x, emb, state], dim=2))
        return shipped(x, t, state, goal)

    net.forward = forward


def run_case(name, OBS, A, TD, T, W, HID, NHID, seed):
    torch.manual_seed(seed)
    ag = object.__new__(ddpm_mod.DiffusionAgent)
    ag.device = "cpu"
    ag.model = Diffusion(state_dim=OBS, action_dim=A, beta_schedule="cosine", n_timesteps=T, loss_type="l2", clip_denoised=True, predict_epsilon=True, device="cpu",
                         model=dict(_target_="agents.models.diffusion.diffusion_models.DiffusionMLPNetwork", action_dim=A, obs_dim=OBS, t_dim=TD, residual_style=True,
                                    hidden_dim=HID, num_hidden_layers=NHID, dropout=0, activation="Mish", use_spectral_norm=False, use_norm=False, device="cpu",
                                    goal_conditioned=False))
    net = ag.model.model
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():      # torch's default initialisation gives a noise estimate far below unit size: values as after training
        for pname, p in net.named_parameters():
            fan_in = p.shape[1] if p.dim() == 2 else 1
            if pname.startswith("layers.layers.%d." % (len(net.layers.layers) - 1)):
                p.copy_(torch.randn(p.shape, generator=g) * ((0.5 / fan_in ** 0.5) if p.dim() == 2 else 0.1))      # a noise estimate of roughly unit size
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / fan_in ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    ag.scaler = make_scaler(OBS, A, seed + 2)
    ag.model.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to("cpu")
    ag.model.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to("cpu")
    ag.window_size, ag.obs_context, ag.diffusion_kde, ag.use_ema = W, deque(maxlen=W), False, False
    sc = ag.scaler
    rng = np.random.default_rng(seed + 3)
    obs = (sc.x_mean.numpy() + rng.normal(size=(N_ENV, T_STEPS, OBS)) * sc.x_std.numpy()).astype(np.float32).astype(np.float64)      # f32 values: predict() rounds its input to f32
    bank = NoiseBank(seed + 4, T, W, A)
    if W > 1:
        with bank:      # as shipped, the second step of an episode (L = 2) cannot run
            ag.reset()
            bank.env = bank.step = bank.call = 0
            ag.predict(obs[0, 0])
            bank.call = 0
            try:
                ag.predict(obs[0, 1])
                raise AssertionError("the shipped DiffusionMLPNetwork ran on a window of two: the repair of case c is not needed any more")
            except RuntimeError as e:
                assert "Sizes of tensors must match" in str(e)
        broadcast_time(net)
    ref32 = rollout(ag, bank, obs, [])
    out = {"%s_sd__%s" % (name, k.replace(".", "__")): v.detach().cpu().numpy() for k, v in ag.model.state_dict().items()}      # (f32, before the second run)
    # ---- the same run in f64: model, schedule, scaling, noise
    ag.model.double()
    schedule_in_f64(ag.model)
    sc.scale_input = lambda x: (x.double() - sc.x_mean.double()) / (sc.x_std.double() + 1e-12)
    bank.dtype = torch.float64
    shipped = ResidualMLPNetwork.forward
    ResidualMLPNetwork.forward = forward_without_cast
    torch.set_default_dtype(torch.float64)      # SinusoidalPosEmb builds its frequencies in the default dtype
    x0_log = []
    try:
        ref64 = rollout(ag, bank, obs, x0_log)
    finally:
        torch.set_default_dtype(torch.float32)
        ResidualMLPNetwork.forward = shipped
    D = float(np.abs(ref32 - ref64).max())
    lo, hi = sc.y_bounds[0], sc.y_bounds[1]
    scaled = (ref64 - sc.y_mean.numpy()) / (sc.y_std.numpy() + 1e-12)
    x0 = np.stack(x0_log)
    inside = float(np.mean((scaled > lo + 1e-6) & (scaled < hi - 1e-6)))
    inside_x0 = float(np.mean((x0 > lo) & (x0 < hi)))
    print("case %s: D = max |f32 - f64| of the reference %.3e (actions of magnitude %.3e); strictly inside the bounds: %.2f of the final action components, %.2f of the x0 "
          "predictions" % (name, D, float(np.abs(ref64).max()), inside, inside_x0))
    populated = int(np.sum(np.abs(ref32 - ref64) > D / 4))
    print("        values that deviate by more than D / 4: %d of %d" % (populated, ref32.size))
    assert 0.3 < inside < 1.0 and 0.2 < inside_x0 < 0.95      # the clamps are exercised and are not all there is
    assert populated >= 8      # D is the maximum over a population, not one value's luck (module docstring)
    out.update({name + "_cfg": np.array([OBS, A, TD, T, W, HID, NHID], dtype=np.int64), name + "_obs": obs, name + "_noise": bank.bank.numpy(), name + "_ref32": ref32,
                name + "_ref64": ref64, name + "_D": np.array(D), name + "_x_mean": sc.x_mean.numpy(), name + "_x_std": sc.x_std.numpy(), name + "_y_mean": sc.y_mean.numpy(),
                name + "_y_std": sc.y_std.numpy(), name + "_y_bounds": sc.y_bounds})
    return out


def main():
    out = {}
    for case in CASES:
        out.update(run_case(*case))
    dst = os.path.join(HERE, "ref_ddpm_mlp_agent.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, "%.0f KB" % (os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
