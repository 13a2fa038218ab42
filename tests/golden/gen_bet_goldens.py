"""Golden vectors for policies.BeTPolicy: the reference's own BeT_Agent (shim-imported, fixed-seed random weights) rolled out batch-1, environment by environment.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_bet_goldens.py
Output (committed): tests/golden/ref_bet_agent.npz - numeric arrays only.  Pins, against the actual reference code:
  * BeT_Agent.predict           (agents/bet_agent.py:328-384)
  * BeT_Policy / MinGPT         (agents/bet_agent.py:23-93, agents/models/bet/latent_generators/mingpt.py:155-186) with GPT (libraries/mingpt/model.py:128-250)
  * KMeansDiscretizer.decode_actions (agents/models/bet/action_ae/discretizers/k_means.py:111-138)
  * Scaler                      (agents/utils/scaler.py:10-113)
The agent is made without BaseAgent.__init__ (no datasets, no k-means fit: the bin centres are random numbers), as gen_agent_goldens.py makes its agents.
torch.multinomial is patched for the run with the inverse-CDF rule of csrc/policy_bet.h - bin = min(#{v : c_v <= u S}, V - 1) on the reference's own probabilities in
f64 - driven by a banked uniform per (environment, step) for the LAST row of the window (the draws of the earlier rows are discarded by the reference, bet_agent.py:364).
A banked u that lies within 1e-4 of an edge of the reference's normalised CDF of its row is drawn again, so every golden bin is decided with a margin far above the
f32 error of a 64-term softmax: the replay tests leave no row out.
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

import agents.bet_agent as bet_mod  # noqa: E402
from agents.models.bet.action_ae.discretizers.k_means import KMeansDiscretizer  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 6, 8
OBS, EMBD, LAYERS, HEADS, WINDOW, V, A = 20, 32, 2, 4, 5, 64, 8
EDGE = 1e-4


def make_scaler(obs_dim, act_dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, obs_dim)) * rng.uniform(0.05, 0.5, obs_dim) + rng.normal(size=obs_dim) * 0.3
    y = rng.normal(size=(400, act_dim)) * 0.004
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


class UniformBank:
    """Patches torch.multinomial(probs [rows, V], 1): row r < rows - 1 takes u = 0.5 (discarded by the reference), the last row the banked u of (env, step)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.u = np.zeros((N_ENV, T_STEPS), dtype=np.float32)
        self.bins = np.zeros((N_ENV, T_STEPS), dtype=np.int64)
        self.redrawn = 0
        self.env = self.step = 0

    def draw(self):
        return np.float32(int(self.rng.integers(0, 1 << 24)) / float(1 << 24))

    @staticmethod
    def rule(c, u):
        return min(int((c <= float(u) * c[-1]).sum()), len(c) - 1)

    def __call__(self, probs, num_samples=1, **kw):
        assert num_samples == 1 and probs.dim() == 2
        out = torch.zeros(probs.shape[0], 1, dtype=torch.long)
        for r in range(probs.shape[0]):
            c = np.cumsum(probs[r].double().numpy())
            u = np.float32(0.5)
            if r == probs.shape[0] - 1:
                u = self.draw()
                while np.abs(float(u) * c[-1] - c).min() / c[-1] < EDGE:
                    u = self.draw(); self.redrawn += 1
                self.u[self.env, self.step] = u
                self.bins[self.env, self.step] = self.rule(c, u)
            out[r, 0] = self.rule(c, u)
        return out

    def __enter__(self):
        self._m = torch.multinomial
        torch.multinomial = self
        return self

    def __exit__(self, *a):
        torch.multinomial = self._m


def sd_arrays(prefix, sd):
    return {prefix + k.replace(".", "__"): v.detach().cpu().numpy() for k, v in sd.items()}


def main():
    torch.manual_seed(11)
    ag = object.__new__(bet_mod.BeT_Agent)
    ag.device = "cpu"
    ag.model = bet_mod.BeT_Policy(
        model=dict(_target_="agents.models.bet.latent_generators.mingpt.MinGPT", discrete_input=False, input_dim=OBS, vocab_size=V, n_layer=LAYERS, n_head=HEADS, n_embd=EMBD,
                   block_size=WINDOW, predict_offsets=True, offset_loss_scale=1.0, focal_loss_gamma=2.0, action_dim=A),
        obs_encoder=dict(_target_="torch.nn.Identity", output_dim=OBS), visual_input=False, device="cpu")
    gpt = ag.model.model.model
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():      # the initialisation (std 0.02, zero biases, unit LayerNorms) makes every bin equally likely: values as after training
        for name, p in gpt.named_parameters():
            if name == "head.weight":
                p[:V] = torch.randn(V, EMBD, generator=g) * 0.35          # logits of standard deviation ~2: neither uniform nor one-hot
                p[V:] = torch.randn(V * A, EMBD, generator=g) * 0.05
            elif name == "pos_emb":
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif ".ln" in name or name.startswith("ln_f"):
                p.copy_((1.0 if name.endswith("weight") else 0.0) + torch.randn(p.shape, generator=g) * (0.2 if name.endswith("weight") else 0.1))
            elif name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.15)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    ag.scaler = make_scaler(OBS, A, 13)
    ag.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to("cpu")
    ag.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to("cpu")
    ag.window_size = WINDOW
    ag.action_ae = KMeansDiscretizer(action_dim=A, num_bins=V, device="cpu", predict_offsets=True)
    ag.action_ae.bin_centers = torch.randn(V, A, generator=g) * 0.9
    ag.obs_context, ag.bp_image_context, ag.inhand_image_context, ag.des_robot_pos_context = (deque(maxlen=WINDOW) for _ in range(4))
    last_logits = []
    gpt.head.register_forward_hook(lambda m, i, o: last_logits.append(o[0, -1, :V].detach().numpy().copy()))
    obs = np.random.default_rng(14).normal(size=(N_ENV, T_STEPS, OBS)) * 0.3
    ref = np.zeros((N_ENV, T_STEPS, A))
    logits = np.zeros((N_ENV, T_STEPS, V), dtype=np.float32)
    bank = UniformBank(15)
    with bank:
        for e in range(N_ENV):
            ag.reset()
            for t in range(T_STEPS):
                bank.env, bank.step = e, t
                ref[e, t] = np.asarray(ag.predict(obs[e, t])).reshape(-1)
                logits[e, t] = last_logits[-1]
    hist = np.bincount(bank.bins.reshape(-1), minlength=V)
    p = torch.softmax(torch.as_tensor(logits), dim=-1).numpy()
    print("bins drawn: %d distinct of %d draws, max probability per row: min %.3f median %.3f max %.3f, redrawn u: %d" % (
        int((hist > 0).sum()), bank.bins.size, p.max(-1).min(), np.median(p.max(-1)), p.max(-1).max(), bank.redrawn))
    assert (hist > 0).sum() > 10 and p.max(-1).max() < 0.95
    out = sd_arrays("bet_sd__", gpt.state_dict())
    out.update(bet_cfg=np.array([OBS, EMBD, LAYERS, HEADS, WINDOW, V, A], dtype=np.int64), bet_centers=ag.action_ae.bin_centers.numpy(), bet_obs=obs, bet_u=bank.u,
               bet_bins=bank.bins, bet_ref=ref, bet_logits=logits, bet_x_mean=ag.scaler.x_mean.numpy(), bet_x_std=ag.scaler.x_std.numpy(),
               bet_y_mean=ag.scaler.y_mean.numpy(), bet_y_std=ag.scaler.y_std.numpy(), bet_y_bounds=ag.scaler.y_bounds)
    dst = os.path.join(HERE, "ref_bet_agent.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, "%.0f KB" % (os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
