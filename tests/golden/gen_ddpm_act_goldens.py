"""Golden vectors for policies.DDPMACTPolicy: the reference's own enc-dec DiffusionAgent + Diffusion + DiffusionEncDec + the act_vae stacks (shim-imported,
fixed-seed weights of trained-like magnitudes) rolled out batch-1, environment by environment.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_ddpm_act_goldens.py
Output (committed): tests/golden/ref_ddpm_act_agent.npz - numeric arrays only.  Pins, against the actual reference code:
  * DiffusionAgent.predict / reset  (agents/ddpm_encdec_agent.py:222-257: the window deque that grows on every step, the chunk counter, inverse scaling)
  * Diffusion.sample                (agents/models/diffusion/diffusion_policy.py:117-217: cosine schedule, epsilon prediction, clipped x0, posterior, final clamp)
  * DiffusionEncDec.forward         (agents/models/diffusion/diffusion_models.py:844-905: time token, pos_emb offsets that follow the window length, encoder, decoder)
  * Scaler                          (agents/utils/scaler.py:10-113)
Two cases at obs 10, A 2, on the shipped network (configs/agents/ddpm_encdec_agent.yaml: width 64, 4 heads, 2 encoder and 4 decoder layers, obs_seq_len 5,
masks of window_size + 1 = 9):
  a: action_seq 4, 16 timesteps, 4 environments x 10 steps, reset() of environment 2 before step 6 - chunks at window lengths 1, 5, 5 and a lane out of phase;
  b: action_seq 2, 4 timesteps, 3 environments x 6 steps - chunks at window lengths 1, 3, 5.
The agent is made without BaseAgent.__init__ (no datasets), use_ema off.  The weights are NOT stored: policies.ddpm_act_synthetic_state draws them from
np.random.RandomState(SEED) over policies.ddpm_act_reference_shapes (asserted here to be the reference model's parameter list, in its order); the fixture keeps their
checksum - the f64 sum of every tensor in sorted key order and a few probed entries.  torch.randn / torch.randn_like are patched for the run to serve a banked normal
per (environment, step, chain index, action token, component): chain index T is the first iterate, index i the noise of reverse step i (the reference draws one at
i = 0 too and multiplies it by zero).

Each case runs TWICE on the same bank: in f32 as shipped, and with model, schedule, scaling and bank in f64.  D = max |f32 - f64| over the emitted actions is the
reference's own f32 error on the case - the yardstick of the replay tests.  Also stored per computed chunk: the f64 iterates of the chain, and the deviation of ONE
f32 reverse step of the reference started from the f64 iterate (teacher-forced) from the f64 result of that step.
"""
import copy
import importlib
import io
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

ref_shims._StubFinder.ROOTS = ref_shims._StubFinder.ROOTS + ("hydra", "omegaconf", "IPython")
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

import agents.ddpm_encdec_agent as encdec_mod  # noqa: E402
from agents.models.diffusion.diffusion_policy import Diffusion  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402
from d3il_amd.policies import ddpm_act_reference_shapes, ddpm_act_synthetic_state, ddpm_schedule  # noqa: E402

OBS, C, HEADS, ENC, DEC, S, A, WINDOW, SEED = 10, 64, 4, 2, 4, 5, 2, 8, 51
CASES = {"a": dict(Ta=4, T=16, n_env=4, n_steps=10, reset_env=2, reset_step=6), "b": dict(Ta=2, T=4, n_env=3, n_steps=6, reset_env=-1, reset_step=-1)}
PROBES = ((0, 0), (3, 1), (17, 5), (40, -1), (77, 2), (100, -3))      # (index into the sorted key list, flat index into that tensor)


def make_scaler(seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, OBS)) * rng.uniform(0.05, 0.5, OBS) + rng.normal(size=OBS) * 0.3
    y = rng.normal(size=(400, A)) * np.array([0.004, 0.006]) + np.array([0.001, -0.002])      # normal data: bounds near +-3 in the scaled space
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


def weight_checksum(sd, keys):
    sums = np.array([float(np.asarray(sd[k], dtype=np.float64).sum()) for k in keys])
    probes = np.array([float(np.asarray(sd[keys[i]]).reshape(-1)[j]) for i, j in PROBES])
    return sums, probes


class NoiseBank:
    """Patches torch.randn / torch.randn_like: call c of a computing predict (c = 0: the first iterate, chain index T; c = 1 + j: reverse step T - 1 - j) returns
    bank[env, step, chain index] in the dtype of the run."""

    def __init__(self, seed, n_env, n_steps, T, Ta):
        self.bank = torch.randn(n_env, n_steps, T + 1, Ta, A, generator=torch.Generator().manual_seed(seed))
        self.T, self.Ta = T, Ta
        self.env = self.step = self.call = 0
        self.dtype = torch.float32

    def take(self, shape):
        assert tuple(shape) == (1, self.Ta, A) and self.call <= self.T
        k = self.T if self.call == 0 else self.T - self.call
        self.call += 1
        return self.bank[self.env, self.step, k].reshape(1, self.Ta, A).to(self.dtype).clone()

    def __enter__(self):
        self._r, self._rl = torch.randn, torch.randn_like
        torch.randn = lambda *s, **k: self.take(s[0] if len(s) == 1 and not isinstance(s[0], int) else s)
        torch.randn_like = lambda x, **k: self.take(x.shape)
        return self

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self._r, self._rl


def schedule_in_f64(d):
    """The reference's schedule attributes, filled with this project's own schedule code (policies.ddpm_schedule) run in f64 on the f32 betas."""
    s = ddpm_schedule(d.betas.double())
    for ref_name, own in (("betas", "betas"), ("alphas", "alphas"), ("alphas_cumprod", "ac"), ("alphas_cumprod_prev", "ac_prev"), ("sqrt_recip_alphas_cumprod", "sqrt_recip_ac"),
                          ("sqrt_recipm1_alphas_cumprod", "sqrt_recipm1_ac"), ("posterior_variance", "post_var"), ("posterior_log_variance_clipped", "post_logvar"),
                          ("posterior_mean_coef1", "coef1"), ("posterior_mean_coef2", "coef2")):
        setattr(d, ref_name, s[own])


def make_agent(Ta, T):
    stack = lambda kind, **kw: dict(_target_="agents.models.act.act_vae." + kind, embed_dim=C, n_heads=HEADS, attn_pdrop=0.1, resid_pdrop=0.1, bias=False, block_size=WINDOW + 1, **kw)
    ag = object.__new__(encdec_mod.DiffusionAgent)
    ag.device = "cpu"
    ag.model = Diffusion(state_dim=OBS, action_dim=A, beta_schedule="cosine", n_timesteps=T, loss_type="l2", clip_denoised=True, predict_epsilon=True, device="cpu",
                         diffusion_x=False, diffusion_x_M=10,
                         model=dict(_target_="agents.models.diffusion.diffusion_models.DiffusionEncDec", state_dim=OBS, action_dim=A, device="cpu", goal_conditioned=False,
                                    goal_seq_len=10, obs_seq_len=S, action_seq_len=Ta, embed_pdrob=0, embed_dim=C, linear_output=True,
                                    encoder=stack("TransformerEncoder", n_layers=ENC), decoder=stack("TransformerDecoder", cross_embed=C, n_layers=DEC)))
    net = ag.model.model
    shapes = ddpm_act_reference_shapes(OBS, A, S, Ta, C, ENC, DEC)
    assert list(shapes.items()) == [(k, tuple(v.shape)) for k, v in net.named_parameters()]      # the project's list is the reference's parameter list, in its order
    sd = ddpm_act_synthetic_state(shapes, SEED)
    full = dict(net.state_dict())      # (its mask buffers stay)
    full.update({k: torch.as_tensor(v) for k, v in sd.items()})
    net.load_state_dict(full)
    ag.model.eval()
    ag.scaler = make_scaler(52)
    ag.model.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to("cpu")
    ag.model.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to("cpu")
    ag.window_size, ag.obs_seq_len, ag.action_seq_size, ag.action_counter = WINDOW, S, Ta, Ta
    ag.obs_context, ag.use_ema, ag.diffusion_kde, ag.goal_condition = deque(maxlen=S), False, False, False
    return ag, sd


def rollout(ag, bank, obs, cfg):
    """(actions, counters after the step, computed flags, window lengths, the current chunk after every step, the iterates [chunk][T + 1] of every computed chunk)."""
    n_env, n_steps, Ta, T = cfg["n_env"], cfg["n_steps"], cfg["Ta"], cfg["T"]
    ref, cnt, computed = np.zeros((n_env, n_steps, A)), np.zeros((n_env, n_steps), dtype=np.int64), np.zeros((n_env, n_steps), dtype=np.int64)
    lens, chunks, iters = np.zeros((n_env, n_steps), dtype=np.int64), np.zeros((n_env, n_steps, Ta, A)), []
    diff = ag.model
    plain = diff.p_sample

    def recording(x, t, s, g, grad=True):
        if int(t[0]) == T - 1:
            iters.append([x.detach().double().numpy().reshape(Ta, A).copy()])
        out = plain(x, t, s, g, grad)
        iters[-1].append(out.detach().double().numpy().reshape(Ta, A).copy())
        return out

    diff.p_sample = recording
    try:
        with bank:
            for e in range(n_env):
                ag.reset()
                for t in range(n_steps):
                    if e == cfg["reset_env"] and t == cfg["reset_step"]:
                        ag.reset()
                    bank.env, bank.step, bank.call = e, t, 0
                    ref[e, t] = np.asarray(ag.predict(obs[e, t])).reshape(-1)
                    assert bank.call in (0, T + 1)
                    cnt[e, t], computed[e, t], lens[e, t] = ag.action_counter, int(bank.call > 0), len(ag.obs_context)
                    chunks[e, t] = ag.curr_action_seq.detach().numpy().reshape(Ta, A)
    finally:
        del diff.p_sample
    return ref, cnt, computed, lens, chunks, np.array(iters)      # iterates [chunk][T + 1 (position p: chain index T - p)][Ta][A]


def run_case(name, cfg):
    Ta, T, n_env, n_steps = cfg["Ta"], cfg["T"], cfg["n_env"], cfg["n_steps"]
    ag, sd = make_agent(Ta, T)
    keys = sorted(sd)
    obs = (np.random.default_rng(53 + ord(name)).normal(size=(n_env, n_steps, OBS)) * 0.3).astype(np.float32)      # predict() rounds its input to f32
    bank = NoiseBank(54 + ord(name), n_env, n_steps, T, Ta)
    ref32, cnt32, comp32, len32, chunks32, it32 = rollout(ag, bank, obs, cfg)
    diff32 = copy.deepcopy(ag.model)
    # ---- the same run in f64: model, schedule, scaling, bounds (already f64), bank
    ag.model.double()
    schedule_in_f64(ag.model)
    sc = ag.scaler
    f32_scale = sc.scale_input
    sc.scale_input = lambda x: (x.double() - sc.x_mean.double()) / (sc.x_std.double() + 1e-12)
    bank.dtype = torch.float64
    torch.set_default_dtype(torch.float64)      # SinusoidalPosEmb builds its frequencies in the default dtype
    ref64, cnt64, comp64, len64, chunks64, it64 = rollout(ag, bank, obs, cfg)
    torch.set_default_dtype(torch.float32)
    assert np.array_equal(cnt32, cnt64) and np.array_equal(comp32, comp64) and np.array_equal(len32, len64)
    D = float(np.abs(ref32 - ref64).max())
    # ---- one f32 reverse step of the reference from the f64 iterate (teacher-forced), per computed chunk and chain step
    sc.scale_input = f32_scale
    step_dev = np.zeros((it64.shape[0], T))
    c = 0
    bank.dtype = torch.float32
    with bank, torch.no_grad():
        for e in range(n_env):
            ctx = deque(maxlen=S)
            for t in range(n_steps):
                if e == cfg["reset_env"] and t == cfg["reset_step"]:
                    ctx.clear()
                ctx.append(sc.scale_input(torch.from_numpy(obs[e, t]).float().unsqueeze(0)))
                if comp64[e, t]:
                    state = torch.stack(tuple(ctx), dim=1)
                    for i in range(T - 1, -1, -1):
                        bank.env, bank.step, bank.call = e, t, T - i
                        x = torch.as_tensor(it64[c, T - 1 - i]).float().reshape(1, Ta, A)
                        out = diff32.p_sample(x, torch.full((1,), i, dtype=torch.long), state, None)
                        step_dev[c, i] = float(np.abs(out.double().numpy().reshape(Ta, A) - it64[c, T - i]).max())
                    c += 1
    assert c == it64.shape[0]
    lo, hi = sc.y_bounds[0], sc.y_bounds[1]
    scale64, shift64 = sc.y_std.numpy() + 1e-12, sc.y_mean.numpy()
    on64 = (((chunks64 - shift64) / scale64) <= lo + 1e-9) | (((chunks64 - shift64) / scale64) >= hi - 1e-9)
    on32 = (((chunks32 - shift64) / scale64) <= lo + 1e-6) | (((chunks32 - shift64) / scale64) >= hi - 1e-6)      # (the f32 run clamps to the bounds rounded to f32)
    sel = comp64 == 1
    assert np.array_equal(on32, on64), "the f32 and the f64 run disagree on which final entries sit on a bound"
    n_on, n_all = int(on64[sel].sum()), int(on64[sel].size)
    assert n_on >= 1 and 2 * (n_all - n_on) >= n_all, (n_on, n_all)
    print("case %s: D = max |f32 - f64| of the reference %.3e (actions of magnitude %.3e); computed chunk entries on a clamp bound: %d of %d; window lengths of the "
          "computed chunks %s; worst teacher-forced f32 step deviation %.3e" % (name, D, float(np.abs(ref64).max()), n_on, n_all, sorted(set(len64[sel].tolist())), step_dev.max()))
    sums, probes = weight_checksum(sd, keys)
    p = "da_%s_" % name
    out = {p + "cfg": np.array([OBS, C, HEADS, ENC, DEC, S, Ta, A, T, WINDOW, SEED, n_env, n_steps, cfg["reset_env"], cfg["reset_step"]], dtype=np.int64), p + "obs": obs,
           p + "noise": bank.bank.numpy(), p + "ref32": ref32, p + "ref64": ref64, p + "counter": cnt32, p + "computed": comp32, p + "len": len32, p + "chunks64": chunks64,
           p + "iter64": it64, p + "step_dev32": step_dev, p + "D": np.array(D), p + "w_sums": sums, p + "w_probes": probes}
    return out, sc


def build():
    out = {}
    for name, cfg in CASES.items():
        part, sc = run_case(name, cfg)
        out.update(part)
    assert out["da_a_computed"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0] and out["da_a_computed"][2].tolist() == [1, 0, 0, 0, 1, 0, 1, 0, 0, 0]
    assert out["da_a_len"][0].tolist() == [1, 2, 3, 4, 5, 5, 5, 5, 5, 5] and out["da_a_len"][2].tolist() == [1, 2, 3, 4, 5, 5, 1, 2, 3, 4]
    assert out["da_b_computed"][0].tolist() == [1, 0, 1, 0, 1, 0] and out["da_b_len"][0].tolist() == [1, 2, 3, 4, 5, 5]
    out.update(da_w_probe_at=np.array(PROBES, dtype=np.int64), da_x_mean=sc.x_mean.numpy(), da_x_std=sc.x_std.numpy(), da_y_mean=sc.y_mean.numpy(), da_y_std=sc.y_std.numpy(),
               da_y_bounds=sc.y_bounds)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    return buf.getvalue()


def main():
    first, second = build(), build()
    assert first == second, "the fixture does not reproduce byte for byte"
    dst = os.path.join(HERE, "ref_ddpm_act_agent.npz")
    with open(dst, "wb") as f:
        f.write(first)
    print("wrote", dst, "%.0f KB" % (os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
