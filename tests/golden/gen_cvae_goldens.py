"""Golden vectors for policies.CVAEPolicy: the reference's own CVAEAgent.predict + VariationalAE + ResidualMLPNetwork + Scaler (shim-imported, fixed-seed weights of
trained-like magnitude) rolled out batch-1, environment by environment, TWICE on the same bank of prior samples - in f32 as shipped, and with model, scaling and
bounds in f64.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_cvae_goldens.py
Output (committed): tests/golden/ref_cvae_agent.npz - numeric arrays only; the file is written with fixed archive timestamps, so a second run reproduces it byte
for byte (``--check`` compares instead of writing).  Pins, against the actual reference code:
  * CVAEAgent.predict            (agents/cvae_agent.py:155-170)
  * VariationalAE.predict        (agents/models/vae/cvae.py:55-62): the prior sample clamped to +-0.5, state first in the decoder's input row
  * ResidualMLPNetwork           (agents/models/common/mlp.py:114-182), Mish, no norm
  * Scaler                       (agents/utils/scaler.py:10-113)
The agent is made without BaseAgent.__init__ (no datasets, no optimiser); min_action / max_action are built as CVAEAgent.__init__ builds them.  torch.randn is
patched to serve a bank stored as f32 (UNCLAMPED standard normals).  D = max |f32 - f64| over the actions is the yardstick of tests/test_policies_cvae.py.

What "f32 as shipped" is (printed by this script, restated by the policy): scale_input returns f32, the decoder runs in f32, ``out.clamp_`` against the float64
bound tensors keeps the f32 output (the comparison is made in f64: the same as clamping against the f32 roundings of the bounds), inverse_scale_output multiplies
by the float64 y_std and adds the float64 y_mean - the returned action is float64, an f64 product and sum on an f32 network output.  For the f64 run
ResidualMLPNetwork.forward's cast to f32 is taken out (the layers are called in order, as forward does), scale_input keeps f64 and the bank is served as f64.
"""
import importlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims._StubFinder.ROOTS = ref_shims._StubFinder.ROOTS + ("hydra", "omegaconf", "tqdm")
ref_shims.install()
import types  # noqa: E402
sys.modules["turtle"] = types.ModuleType("turtle")      # cvae.py starts with a stray `from turtle import forward`, which would pull in tkinter
sys.modules["turtle"].forward = None
import hydra  # noqa: E402  (stub)


class Cfg(dict):
    """A dict with attribute access, as VariationalAE.__init__ reads its DictConfig (encoder.latent_dim, encoder.model_config.hidden_dim)."""
    __getattr__ = dict.__getitem__


def instantiate(cfg, *args, **kwargs):
    cfg = Cfg(cfg)
    target = cfg.pop("_target_")
    cfg.pop("_recursive_", None)
    mod, name = target.rsplit(".", 1)
    cfg.update(kwargs)
    return getattr(importlib.import_module(mod), name)(*args, **cfg)


hydra.utils.instantiate = instantiate

import agents.cvae_agent as cvae_mod  # noqa: E402
from agents.models.vae.cvae import VariationalAE  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 4, 4
OBS, A, HIDDEN, LAYERS, L = 6, 2, 128, 2, 16
OUT_GAIN = 1.7      # the output layer's gain: decoder outputs of a few units, so that some but not all reach the action clamp (the bounds sit near +-3)


def make_scaler(seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, OBS)) * rng.uniform(0.05, 0.5, OBS) + rng.normal(size=OBS) * 0.3
    y = rng.normal(size=(400, A)) * 0.004 + rng.normal(size=A) * 0.002
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


def make_agent():
    ag = object.__new__(cvae_mod.CVAEAgent)
    ag.device = "cpu"
    torch.manual_seed(31)
    mlp = dict(_target_="agents.models.common.mlp.ResidualMLPNetwork", hidden_dim=HIDDEN, num_hidden_layers=LAYERS, dropout=0, activation="Mish", use_spectral_norm=False,
               device="cpu")
    ag.model = VariationalAE(
        encoder=Cfg(_target_="agents.models.vae.cvae.VariationalEncoder", _recursive_=False, latent_dim=L, device="cpu", model_config=Cfg(mlp, input_dim=OBS + A)),
        decoder=Cfg(_target_="agents.models.common.mlp.ResidualMLPNetwork", _recursive_=False, input_dim=OBS, output_dim=A, dropout=0, activation="Mish", use_spectral_norm=False,
                    use_norm=False, norm_style="BatchNorm", device="cpu"),
        device="cpu")
    g = torch.Generator().manual_seed(32)
    last = "layers.%d." % (len(ag.model.decoder.layers) - 1)
    with torch.no_grad():      # values as after training
        for name, p in ag.model.decoder.named_parameters():
            gain = OUT_GAIN if name.startswith(last) else 1.0
            p.copy_(torch.randn(p.shape, generator=g) * (gain * (2.0 / p.shape[1]) ** 0.5 if name.endswith("weight") else 0.1))
    ag.scaler = make_scaler(33)
    ag.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to(ag.device)      # cvae_agent.py:46-47
    ag.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to(ag.device)
    return ag


class Bank:
    def __init__(self, seed):
        self.z = np.random.default_rng(seed).normal(size=(N_ENV, T_STEPS, L)).astype(np.float32)
        self.env = self.step = self.calls = 0
        self.f64 = False

    def randn(self, *size, **kw):
        size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        assert size == (1, L), size
        self.calls += 1
        return torch.as_tensor(self.z[self.env, self.step]).to(torch.float64 if self.f64 else torch.float32).reshape(1, L)


def run(ag, bank, obs, f64):
    """The 16 predict calls; returns (actions [N, T, A], decoder outputs before the clamp [N, T, A], decoder inputs [N, T, OBS + L]) as f64 arrays and what dtypes were seen."""
    dec = ag.model.decoder
    seen = []
    hook = dec.register_forward_hook(lambda m, i, o: seen.append((i[0].detach().clone(), o.detach().clone())))
    keep = (torch.randn, ag.scaler.scale_input)
    torch.randn = bank.randn
    bank.f64 = f64
    if f64:
        ag.model.double()
        sc = ag.scaler
        sc.scale_input = lambda x: (x.double().to(sc.device) - sc.x_mean) / (sc.x_std + 1e-12)
        def forward(x):      # ResidualMLPNetwork.forward without its cast to f32
            for layer in dec.layers:
                x = layer(x)
            return x
        dec.forward = forward
    out = (np.zeros((N_ENV, T_STEPS, A)), np.zeros((N_ENV, T_STEPS, A)), np.zeros((N_ENV, T_STEPS, OBS + L)))
    try:
        for e in range(N_ENV):
            for t in range(T_STEPS):
                bank.env, bank.step = e, t
                calls = bank.calls
                y = ag.predict(obs[e, t])
                assert bank.calls == calls + 1
                xin, raw = seen[-1]
                out[0][e, t] = np.asarray(y, dtype=np.float64).reshape(-1)
                out[1][e, t], out[2][e, t] = raw.double().numpy().reshape(A), xin.double().numpy().reshape(OBS + L)
    finally:
        hook.remove()
        torch.randn = keep[0]
        if f64:
            ag.scaler.scale_input = keep[1]
            del dec.forward
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
    sd = {k: v.detach().clone() for k, v in ag.model.decoder.state_dict().items()}
    lo, hi = ag.scaler.y_bounds[0].copy(), ag.scaler.y_bounds[1].copy()
    bank = Bank(34)
    rng = np.random.default_rng(35)
    obs = (ag.scaler.x_mean.numpy() + rng.normal(size=(N_ENV, T_STEPS, OBS)) * ag.scaler.x_std.numpy()).astype(np.float32)
    r64, dt64 = run(ag, bank, obs, True)
    r32, dt32 = run(ag, bank, obs, False)
    assert all(torch.equal(sd[k], v) for k, v in ag.model.decoder.state_dict().items())
    D = float(np.abs(r32[0] - r64[0]).max())
    zc = np.clip(bank.z.astype(np.float64), -0.5, 0.5)
    assert np.array_equal(r64[2][:, :, OBS:], zc) and np.array_equal(r32[2][:, :, OBS:], zc)      # state first, the clamped latent second
    hit = (r64[1] < lo) | (r64[1] > hi)
    print("dtypes of (decoder input, decoder output, returned action): shipped run %s, f64 run %s; min_action %s, y_std %s" % (dt32, dt64, ag.min_action.dtype, ag.scaler.y_std.dtype))
    print("D = %.3e (largest |action - y_mean| %.3e); decoder outputs %.2f .. %.2f, bounds %s .. %s; outputs past a bound: %d of %d (f32 run: %d); latent components on a bound: %d of %d"
          % (D, float(np.abs(r64[0] - ag.scaler.y_mean.numpy()).max()), r64[1].min(), r64[1].max(), np.round(lo, 2), np.round(hi, 2), int(hit.sum()), hit.size,
             int(((r32[1] < lo) | (r32[1] > hi)).sum()), int((np.abs(bank.z) >= 0.5).sum()), bank.z.size))
    assert 0 < hit.sum() < hit.size
    # clamping the f32 output against the f64 bounds equals clamping against their f32 roundings; the action is the f64 product and sum on that
    raw32 = r32[1].astype(np.float32)
    c32 = np.minimum(np.maximum(raw32, lo.astype(np.float32)), hi.astype(np.float32)).astype(np.float64)
    assert np.array_equal(c32 * (ag.scaler.y_std.numpy() + 1e-12) + ag.scaler.y_mean.numpy(), r32[0])
    out = {"cvae_sd__" + k.replace(".", "__"): v.numpy() for k, v in sd.items()}
    out.update(cvae_cfg=np.array([OBS, A, HIDDEN, LAYERS, L], dtype=np.int64), cvae_obs=obs, cvae_z=bank.z,
               cvae_x_mean=ag.scaler.x_mean.numpy(), cvae_x_std=ag.scaler.x_std.numpy(), cvae_y_mean=ag.scaler.y_mean.numpy(), cvae_y_std=ag.scaler.y_std.numpy(), cvae_y_bounds=ag.scaler.y_bounds,
               cvae_ref32=r32[0], cvae_raw32=r32[1].astype(np.float32), cvae_ref64=r64[0], cvae_raw64=r64[1], cvae_in64=r64[2], cvae_D=np.array([D]))
    data = npz_bytes(out)
    dst = os.path.join(HERE, "ref_cvae_agent.npz")
    if "--check" in sys.argv:
        same = open(dst, "rb").read() == data
        print("the committed file is reproduced byte for byte" if same else "the committed file DIFFERS from this run")
        sys.exit(0 if same else 1)
    with open(dst, "wb") as f:
        f.write(data)
    print("wrote", dst, "%.0f KB" % (len(data) / 1024))


if __name__ == "__main__":
    main()
