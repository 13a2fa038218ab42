"""Golden vectors for policies.ACTPolicy: the reference's own ActAgent + ActVAE (shim-imported, fixed-seed weights of trained-like magnitudes) rolled out batch-1,
environment by environment.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_act_goldens.py
Output (committed): tests/golden/ref_act_agent.npz - numeric arrays only.  Pins, against the actual reference code:
  * ActAgent.predict / reset   (agents/act_agent.py:207-239: the chunk counter, clamp to the scaler's bounds, inverse scaling)
  * ActVAE.forward, no actions (agents/models/act/act_vae.py:389-445: uniform latent, encoder with its causal mask, decoder with self + cross attention)
  * Scaler                     (agents/utils/scaler.py:10-113)
The shipped configuration (configs/agents/act_agent.yaml): 2 encoder and 4 decoder layers, width 64, 4 heads, latent 32; T = 3, obs 10, A = 2.  The agent is made
without BaseAgent.__init__ (no datasets).  The weights used at inference are 1.4 MB and are NOT stored: policies.act_synthetic_state draws them from
np.random.RandomState(SEED) over policies.act_reference_shapes (asserted here to be the reference model's parameter list); the fixture keeps their checksum - the f64
sum of every tensor in sorted key order and a few probed entries.  torch.rand is patched for the run to serve a banked f32 latent per (environment, step).

4 environments x 7 steps: chunk boundaries at steps 0, 3 and 6, and a reset() of environment RESET_ENV before step RESET_STEP, which lands mid-chunk.  The reference
runs TWICE on the same bank: in f32 as shipped, and with model, scaling and bounds in f64.  D = max |f32 - f64| over the emitted actions is the reference's own f32
error on this problem - the yardstick of the replay tests.
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

import agents.act_agent as act_mod  # noqa: E402
from agents.models.act.act_vae import ActVAE  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402
from d3il_amd.policies import act_reference_shapes, act_synthetic_state  # noqa: E402

N_ENV, N_STEPS, RESET_ENV, RESET_STEP = 4, 7, 2, 4
OBS, C, HEADS, ENC, DEC, LAT, T, A, SEED = 10, 64, 4, 2, 4, 32, 3, 2, 41
PROBES = ((0, 0), (3, 1), (17, 5), (40, -1), (77, 2), (120, -3))      # (index into the sorted key list, flat index into that tensor)


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def stack_cfg(kind, **kw):
    return AttrDict(_target_="agents.models.act.act_vae." + kind, embed_dim=C, n_heads=HEADS, attn_pdrop=0.1, resid_pdrop=0.1, bias=False, **kw)


def make_scaler(seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, OBS)) * rng.uniform(0.05, 0.5, OBS) + rng.normal(size=OBS) * 0.3
    y = rng.uniform(-1.0, 1.0, size=(400, A)) * np.array([0.004, 0.006]) + np.array([0.001, -0.002])      # uniform data: bounds near +-sqrt(3) in the scaled space
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


def weight_checksum(sd, keys):
    sums = np.array([float(np.asarray(sd[k], dtype=np.float64).sum()) for k in keys])
    probes = np.array([float(np.asarray(sd[keys[i]]).reshape(-1)[j]) for i, j in PROBES])
    return sums, probes


class LatentBank:
    """Patches torch.rand: the one call of a computing predict returns bank[env, step] in the dtype of the run."""

    def __init__(self, seed):
        self.bank = torch.rand(N_ENV, N_STEPS, LAT, generator=torch.Generator().manual_seed(seed))
        self.env = self.step = self.calls = 0
        self.dtype = torch.float32

    def take(self, shape):
        assert tuple(shape) == (1, 1, LAT)
        self.calls += 1
        return self.bank[self.env, self.step].reshape(1, 1, LAT).to(self.dtype).clone()

    def __enter__(self):
        self._r = torch.rand
        torch.rand = lambda *s, **k: self.take(s[0] if len(s) == 1 and not isinstance(s[0], int) else s)
        return self

    def __exit__(self, *a):
        torch.rand = self._r


def rollout(ag, bank, obs):
    ref, cnt, computed = np.zeros((N_ENV, N_STEPS, A)), np.zeros((N_ENV, N_STEPS), dtype=np.int64), np.zeros((N_ENV, N_STEPS), dtype=np.int64)
    chunks = np.zeros((N_ENV, N_STEPS, T, A))
    with bank:
        for e in range(N_ENV):
            ag.reset()
            for t in range(N_STEPS):
                if e == RESET_ENV and t == RESET_STEP:
                    ag.reset()
                bank.env, bank.step, before = e, t, bank.calls
                ref[e, t] = np.asarray(ag.predict(obs[e, t])).reshape(-1)
                cnt[e, t], computed[e, t] = ag.action_counter, bank.calls - before
                chunks[e, t] = ag.curr_action_seq.detach().numpy().reshape(T, A)
    return ref, cnt, computed, chunks


def main():
    ag = object.__new__(act_mod.ActAgent)
    ag.device = "cpu"
    ag.model = ActVAE(action_encoder=stack_cfg("TransformerEncoder", n_layers=2, block_size=T + 1), encoder=stack_cfg("TransformerEncoder", n_layers=ENC, block_size=T),
                      decoder=stack_cfg("TransformerDecoder", cross_embed=C, n_layers=DEC, block_size=T), state_dim=OBS, action_dim=A, hidden_dim=C, act_seq_size=T,
                      latent_dim=LAT)
    shapes = act_reference_shapes(OBS, A, T, C, ENC, DEC, LAT, 2)
    assert shapes == {k: tuple(v.shape) for k, v in ag.model.named_parameters()}      # the project's list is the reference's parameter list
    sd = act_synthetic_state(shapes, SEED)
    keys = sorted(sd)
    full = dict(ag.model.state_dict())      # (its mask buffers stay)
    full.update({k: torch.as_tensor(v) for k, v in sd.items()})
    ag.model.load_state_dict(full)
    ag.model.eval()
    ag.scaler = make_scaler(42)
    ag.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to("cpu")
    ag.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to("cpu")
    ag.action_seq_size, ag.obs_size, ag.window_size, ag.gc = T, 1, T, False
    ag.action_counter = T
    obs = (np.random.default_rng(43).normal(size=(N_ENV, N_STEPS, OBS)) * 0.3).astype(np.float32)      # predict() rounds its input to f32
    bank = LatentBank(44)
    ref32, cnt32, comp32, chunks32 = rollout(ag, bank, obs)
    # ---- the same run in f64: model, scaling, bounds (already f64), latent
    ag.model.double()
    sc = ag.scaler
    sc.scale_input = lambda x: (x.double() - sc.x_mean.double()) / (sc.x_std.double() + 1e-12)
    bank.dtype = torch.float64
    torch.set_default_dtype(torch.float64)
    ref64, cnt64, comp64, chunks64 = rollout(ag, bank, obs)
    torch.set_default_dtype(torch.float32)
    assert np.array_equal(cnt32, cnt64) and np.array_equal(comp32, comp64)
    assert comp32[0].tolist() == [1, 0, 0, 1, 0, 0, 1] and comp32[RESET_ENV].tolist() == [1, 0, 0, 1, 1, 0, 0]
    D = float(np.abs(ref32 - ref64).max())
    lo, hi = sc.y_bounds[0], sc.y_bounds[1]
    scaled = (chunks64[comp64 == 1] - sc.y_mean.numpy()) / (sc.y_std.numpy() + 1e-12)      # the chunks as computed, in the scaled space
    on = int(((scaled <= lo + 1e-9) | (scaled >= hi - 1e-9)).sum())
    print("D = max |f32 - f64| of the reference: %.3e (actions of magnitude %.3e); chunk entries on a clamp bound: %d, inside: %d" % (D, float(np.abs(ref64).max()), on, scaled.size - on))
    assert on > 0 and scaled.size - on > on
    sums, probes = weight_checksum(sd, keys)
    out = dict(act_cfg=np.array([OBS, C, HEADS, ENC, DEC, LAT, T, A, SEED, RESET_ENV, RESET_STEP], dtype=np.int64), act_obs=obs, act_latent=bank.bank.numpy(), act_ref32=ref32,
               act_ref64=ref64, act_counter=cnt32, act_computed=comp32, act_chunks64=chunks64, act_D=np.array(D), act_w_sums=sums, act_w_probes=probes,
               act_w_probe_at=np.array(PROBES, dtype=np.int64), act_x_mean=sc.x_mean.numpy(), act_x_std=sc.x_std.numpy(), act_y_mean=sc.y_mean.numpy(), act_y_std=sc.y_std.numpy(),
               act_y_bounds=sc.y_bounds)
    dst = os.path.join(HERE, "ref_act_agent.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, "%.0f KB" % (os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
