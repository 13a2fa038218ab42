"""Golden vectors for policies.BeTMLPPolicy: the reference's own BetMLP_Agent.predict + BeTPolicy.generate_latents + ResidualMLPNetwork + KMeansDiscretizer + Scaler
(shim-imported, fixed-seed weights of trained-like magnitude) rolled out batch-1, environment by environment, TWICE on the same bank of uniforms - in f32 as shipped,
and with model, scaling, bin centres and bounds in f64.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_bet_mlp_goldens.py
Output (committed): tests/golden/ref_bet_mlp_agent.npz - numeric arrays only; the file is written with fixed archive timestamps, so a second run reproduces it byte
for byte (``--check`` compares instead of writing).  Pins, against the actual reference code:
  * BetMLP_Agent.predict         (agents/bet_mlp_agent.py:366-406): no history, a [1, 1, obs] row
  * BeTPolicy.generate_latents   (same file, 114-147): logits = out[:V], offsets in the layout "(V A)"
  * ResidualMLPNetwork           (agents/models/common/mlp.py:114-189), Mish, no norm, an output layer with bias
  * KMeansDiscretizer.decode_actions (agents/models/bet/action_ae/discretizers/k_means.py:111-138)
  * Scaler                       (agents/utils/scaler.py:10-113)
The agent is made without BaseAgent.__init__ (no datasets, no k-means fit: the bin centres are random numbers); min_action / max_action are built as
BetMLP_Agent.__init__ builds them.  torch.multinomial is patched with the inverse-CDF rule of csrc/policy_bet_mlp.h - bin = min(#{v : c_v <= u S}, V - 1) on the
reference's own probabilities in f64 - driven by a banked uniform per (environment, step).  A banked u that lies within EDGE of an edge of the normalised f64 CDF of
its row - in the f64 run, which is made first and fixes the bank - is drawn again, so every golden bin is decided with a margin far above the f32 error of a 64-term
softmax (printed: the largest deviation of the shipped run's f32 normalised CDF from the f64 one, which has to stay below EDGE / 4): the replay tests leave no row
out.  D = max |f32 - f64| over the actions is the yardstick of tests/test_policies_bet_mlp.py.

What "f32 as shipped" is (printed by this script, restated by the policy): scale_input returns f32, the network runs in f32, bin_centers[bin] + offset is an f32
sum, ``actions.clamp_`` against the float64 bound tensors keeps the f32 sum (the comparison is made in f64: the same as clamping against the f32 roundings of the
bounds), inverse_scale_output multiplies by the float64 y_std and adds the float64 y_mean - the returned action is float64, an f64 product and sum on an f32 value.
For the f64 run ResidualMLPNetwork.forward's cast to f32 is taken out (the layers are called in order, as forward does), scale_input keeps f64 and the bin centres
are f64.
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

import agents.bet_mlp_agent as bm_mod  # noqa: E402
from agents.models.bet.action_ae.discretizers.k_means import KMeansDiscretizer  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 6, 4
OBS, A, HIDDEN, LAYERS, V = 6, 2, 128, 2, 64
EDGE = 1e-4


def make_scaler(seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, OBS)) * rng.uniform(0.05, 0.5, OBS) + rng.normal(size=OBS) * 0.3
    y = rng.normal(size=(400, A)) * 0.004 + rng.normal(size=A) * 0.002
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


def make_agent():
    ag = object.__new__(bm_mod.BetMLP_Agent)
    ag.device = "cpu"
    torch.manual_seed(41)
    ag.model = bm_mod.BeTPolicy(
        model=dict(_target_="agents.models.common.mlp.ResidualMLPNetwork", input_dim=OBS, hidden_dim=HIDDEN, num_hidden_layers=LAYERS, dropout=0, activation="Mish",
                   use_spectral_norm=False, use_norm=False, norm_style="BatchNorm", device="cpu"),
        obs_dim=OBS, act_dim=A, vocab_size=V, predict_offsets=True, focal_loss_gamma=2.0, offset_loss_scale=1.0, device="cpu")
    net = ag.model.model
    g = torch.Generator().manual_seed(42)
    last = "layers.%d." % (len(net.layers) - 1)
    with torch.no_grad():      # values as after training
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p.shape[1]) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        w = net.get_parameter(last + "weight")
        w[:V] *= 0.75      # logits of standard deviation ~2: neither uniform nor one-hot
        w[V:] *= 0.35      # offsets of a few tenths next to centres of 0.9: some sums reach the action clamp (the bounds sit near +-3), most do not
    ag.scaler = make_scaler(43)
    ag.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to(ag.device)      # bet_mlp_agent.py:176-177
    ag.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to(ag.device)
    ag.window_size = 1
    ag.obs_encoding_net = torch.nn.Identity()
    ag.action_ae = KMeansDiscretizer(action_dim=A, num_bins=V, device="cpu", predict_offsets=True)
    ag.action_ae.bin_centers = torch.randn(V, A, generator=g) * 1.6
    ag.obs_context = deque(maxlen=1)
    return ag, g


class UniformBank:
    """Patches torch.multinomial(probs [1, V], 1).  ``fix``: draw a fresh u per call and draw again inside EDGE of the row's f64 CDF (the f64 run); afterwards the
    bank is served as it stands (the shipped run)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.u = np.zeros((N_ENV, T_STEPS), dtype=np.float32)
        self.redrawn = self.calls = 0
        self.env = self.step = 0
        self.fix = True
        self.bins, self.cdf = {}, {}

    def draw(self):
        return np.float32(int(self.rng.integers(0, 1 << 24)) / float(1 << 24))

    @staticmethod
    def rule(c, u):
        return min(int((c <= float(u) * c[-1]).sum()), len(c) - 1)

    def __call__(self, probs, num_samples=1, **kw):
        assert num_samples == 1 and tuple(probs.shape) == (1, V)
        self.calls += 1
        c = np.cumsum(probs[0].double().numpy())
        if self.fix:
            u = self.draw()
            while np.abs(float(u) * c[-1] - c).min() / c[-1] < EDGE:
                u = self.draw(); self.redrawn += 1
            self.u[self.env, self.step] = u
        u = self.u[self.env, self.step]
        key = (self.fix, self.env, self.step)
        self.bins[key], self.cdf[key] = self.rule(c, u), c / c[-1]
        return torch.full((1, 1), self.bins[key], dtype=torch.long)

    def __enter__(self):
        self._m = torch.multinomial
        torch.multinomial = self
        return self

    def __exit__(self, *a):
        torch.multinomial = self._m


def run(ag, bank, obs, f64):
    """The 24 predict calls; returns (actions [N, T, A], network outputs [N, T, V (1 + A)], bins [N, T]) and the dtypes seen."""
    net = ag.model.model
    seen = []
    hook = net.register_forward_hook(lambda m, i, o: seen.append((i[0].detach().clone(), o.detach().clone())))
    keep = (ag.scaler.scale_input, ag.action_ae.bin_centers)
    bank.fix = f64
    if f64:
        net.double()
        sc = ag.scaler
        sc.scale_input = lambda x: (x.double().to(sc.device) - sc.x_mean) / (sc.x_std + 1e-12)
        def forward(x):      # ResidualMLPNetwork.forward without its cast to f32
            for layer in net.layers:
                x = layer(x)
            return x
        net.forward = forward
        ag.action_ae.bin_centers = keep[1].double()
    out = (np.zeros((N_ENV, T_STEPS, A)), np.zeros((N_ENV, T_STEPS, V * (1 + A))), np.zeros((N_ENV, T_STEPS), dtype=np.int64))
    try:
        with bank:
            for e in range(N_ENV):
                ag.reset()
                for t in range(T_STEPS):
                    bank.env, bank.step = e, t
                    calls = bank.calls
                    y = ag.predict(obs[e, t])
                    assert bank.calls == calls + 1
                    xin, raw = seen[-1]
                    assert tuple(xin.shape) == (1, 1, OBS)
                    out[0][e, t] = np.asarray(y, dtype=np.float64).reshape(-1)
                    out[1][e, t] = raw.double().numpy().reshape(-1)
                    out[2][e, t] = bank.bins[(f64, e, t)]
    finally:
        hook.remove()
        if f64:
            ag.scaler.scale_input, ag.action_ae.bin_centers = keep
            del net.forward
            net.float()
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
    ag, _ = make_agent()
    net = ag.model.model
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    centers = ag.action_ae.bin_centers.clone()
    lo, hi = ag.scaler.y_bounds[0].copy(), ag.scaler.y_bounds[1].copy()
    bank = UniformBank(44)
    rng = np.random.default_rng(45)
    obs = (ag.scaler.x_mean.numpy() + rng.normal(size=(N_ENV, T_STEPS, OBS)) * ag.scaler.x_std.numpy()).astype(np.float32)
    r64, dt64 = run(ag, bank, obs, True)
    r32, dt32 = run(ag, bank, obs, False)
    assert all(torch.equal(sd[k], v) for k, v in net.state_dict().items()) and torch.equal(centers, ag.action_ae.bin_centers)
    assert np.array_equal(r32[2], r64[2]), "a bin differs between the shipped and the f64 run: EDGE is too small"
    cdf_dev = max(float(np.abs(bank.cdf[(False, e, t)] - bank.cdf[(True, e, t)]).max()) for e in range(N_ENV) for t in range(T_STEPS))
    D = float(np.abs(r32[0] - r64[0]).max())
    logits = r64[1][:, :, :V]
    p = np.exp(logits - logits.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    hist = np.bincount(r64[2].reshape(-1), minlength=V)
    bins = r64[2]
    off64 = r64[1][:, :, V:].reshape(N_ENV, T_STEPS, V, A)[np.arange(N_ENV)[:, None], np.arange(T_STEPS)[None, :], bins]
    v64 = centers.double().numpy()[bins] + off64
    hit = (v64 < lo) | (v64 > hi)
    print("dtypes of (network input, network output, returned action): shipped run %s, f64 run %s; min_action %s, y_std %s, bin_centers %s"
          % (dt32, dt64, ag.min_action.dtype, ag.scaler.y_std.dtype, centers.dtype))
    print("D = %.3e (largest |action - y_mean| %.3e); logits: standard deviation %.2f, max probability per row min %.3f median %.3f max %.3f; bins drawn: %d distinct of %d; "
          "redrawn u: %d; EDGE %.1e, f32 CDF against f64 CDF %.3e (EDGE / 4 = %.1e); centre + offset past a bound: %d of %d"
          % (D, float(np.abs(r64[0] - ag.scaler.y_mean.numpy()).max()), float(logits.std(-1).mean()), p.max(-1).min(), np.median(p.max(-1)), p.max(-1).max(),
             int((hist > 0).sum()), bins.size, bank.redrawn, EDGE, cdf_dev, EDGE / 4, int(hit.sum()), hit.size))
    assert (hist > 0).sum() > 10 and p.max(-1).max() < 0.95 and 1.5 < logits.std(-1).mean() < 2.5
    assert cdf_dev < EDGE / 4
    assert 0 < hit.sum() < hit.size
    # the shipped arithmetic, restated: f32 sum, clamp against the f32 roundings of the bounds, f64 product and sum
    raw32 = r32[1].astype(np.float32)
    off32 = raw32[:, :, V:].reshape(N_ENV, T_STEPS, V, A)[np.arange(N_ENV)[:, None], np.arange(T_STEPS)[None, :], bins]
    v32 = (centers.numpy()[bins] + off32).astype(np.float32)
    c32 = np.minimum(np.maximum(v32, lo.astype(np.float32)), hi.astype(np.float32)).astype(np.float64)
    eps = np.float64(np.float32(1e-12))      # (the scaler adds 1e-12 * torch.ones(..): an f32 tensor)
    assert np.array_equal(c32 * (ag.scaler.y_std.numpy() + eps) + ag.scaler.y_mean.numpy(), r32[0])
    out = {"bm_sd__" + k.replace(".", "__"): v.numpy() for k, v in sd.items()}
    out.update(bm_cfg=np.array([OBS, A, HIDDEN, LAYERS, V], dtype=np.int64), bm_obs=obs, bm_u=bank.u, bm_bins=bins, bm_centers=centers.numpy(),
               bm_x_mean=ag.scaler.x_mean.numpy(), bm_x_std=ag.scaler.x_std.numpy(), bm_y_mean=ag.scaler.y_mean.numpy(), bm_y_std=ag.scaler.y_std.numpy(), bm_y_bounds=ag.scaler.y_bounds,
               bm_ref32=r32[0], bm_raw32=raw32, bm_ref64=r64[0], bm_raw64=r64[1], bm_D=np.array([D]), bm_edge=np.array([EDGE, cdf_dev]))
    data = npz_bytes(out)
    dst = os.path.join(HERE, "ref_bet_mlp_agent.npz")
    if "--check" in sys.argv:
        same = open(dst, "rb").read() == data
        print("the committed file is reproduced byte for byte" if same else "the committed file DIFFERS from this run")
        sys.exit(0 if same else 1)
    with open(dst, "wb") as f:
        f.write(data)
    print("wrote", dst, "%.0f KB" % (len(data) / 1024))


if __name__ == "__main__":
    main()
