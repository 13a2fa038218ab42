"""Golden vectors for policies.BCGMMPolicy: the reference's own BC_GMM + ResidualMLPNetwork + Scaler under BC_Agent.predict (shim-imported, fixed-seed weights of
trained-like magnitude) rolled out batch-1, environment by environment, TWICE on the same bank of uniforms and normals - in f32 as shipped, and with model,
scaling and bounds in f64.  Three cases: (a) the avoiding script's shape (obs 4, A 2, G 8, low-noise, hidden 128 / 2 layers: a kernel shape), (b) G 64, A 3, obs 20,
``exp`` std with low_noise_eval off, hidden 32 / 4 layers (the torch path), (c) G 24, A 8, ``softplus``, hidden 128 / 2 layers.

Run where the reference is only (its path: D3IL_REFERENCE, tests/golden/ref_shims.py):  python tests/golden/gen_bc_gmm_goldens.py
Output (committed): tests/golden/ref_bc_gmm_agent.npz - numeric arrays only; the file is written with fixed archive timestamps, so a second run reproduces it byte
for byte (``--check`` compares instead of writing).  Pins, against the actual reference code:
  * BC_GMM                       (agents/models/gmm/bc_gmm.py:13-90): Mish behind the ResidualMLP's own output layer, 0.01 tanh on the means, the std switch, layout "(G A)"
  * ResidualMLPNetwork           (agents/models/common/mlp.py:114-189), Mish, no norm
  * MixtureSameFamily.sample     (torch): ONE torch.multinomial call on [1, G], ONE torch.normal call on [1, 1, G, A], the drawn component's A values kept
  * BC_Agent.predict             (agents/bc_agent.py:240-271): a [1, 1, obs] row, clamp_ against the f64 bounds, the f64 inverse scaling
  * Scaler                       (agents/utils/scaler.py:10-113)
The reference has no agents/bc_gmm_agent.py (its yaml names one): BC_Agent.predict is handed a thin module of this file whose forward is ``gmm(x).sample()``; the
agent is made without BaseAgent.__init__ (no datasets), min_action / max_action as BC_Agent.__init__ builds them.  torch.multinomial is patched with the
inverse-CDF rule of csrc/policy_bc_gmm.h - k = min(#{g : c_g <= u S}, G - 1) on the reference's own probabilities in f64 - driven by a banked uniform per
(environment, step); a banked u within EDGE of an edge of the row's normalised f64 CDF - in the f64 run, which is made first and fixes the bank - is drawn again,
so that the replay tests leave no row out.  torch.normal is patched to loc + scale * Z with the banked z [A] placed at every component.
D = max |f32 - f64| over the actions, per case, is the yardstick of tests/test_policies_bc_gmm.py.
"""
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

ref_shims._StubFinder.ROOTS = ref_shims._StubFinder.ROOTS + ("hydra", "omegaconf", "tqdm", "torchsde", "torchdiffeq")
ref_shims.install()

import agents.bc_agent as bc_mod  # noqa: E402
from agents.models.gmm.bc_gmm import BC_GMM  # noqa: E402
from agents.utils.scaler import Scaler  # noqa: E402

N_ENV, T_STEPS = 6, 4
EDGE = 1e-4
#        name  obs  A   G  hidden layers std_activation low_noise  spread of the action data (scaled bounds follow from it)
CASES = (("a", 4, 2, 8, 128, 2, "exp", True, "normal"),
         ("b", 20, 3, 64, 32, 4, "exp", False, "uniform"),
         ("c", 10, 8, 24, 128, 2, "softplus", False, "normal"))
MIN_STD = 1e-4


class SampleOnce(torch.nn.Module):
    """What a BC_GMM_Agent would hand BC_Agent.predict: the mixture sampled once per call."""

    def __init__(self, gmm):
        super().__init__()
        self.gmm = gmm

    def forward(self, x):
        return self.gmm(x).sample()


def make_scaler(seed, obs, A, spread):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(400, obs)) * rng.uniform(0.05, 0.5, obs) + rng.normal(size=obs) * 0.3
    # "uniform" action data: the scaled bounds sit at +-sqrt(3) = 1.73, which a sample of mean + std z with std around exp(-0.5) passes now and then
    y = (rng.uniform(-1, 1, size=(400, A)) if spread == "uniform" else rng.normal(size=(400, A))) * 0.004 + rng.normal(size=A) * 0.002
    return Scaler(x.astype(np.float64), y.astype(np.float64), True, "cpu")


def make_agent(idx, obs, A, G, hidden, layers, act, low, spread):
    ag = object.__new__(bc_mod.BC_Agent)
    ag.device = "cpu"
    torch.manual_seed(60 + idx)
    gmm = BC_GMM(input_dim=obs, hidden_dim=hidden, num_hidden_layers=layers, mlp_output_dim=hidden, dropout=0, activation="Mish", use_spectral_norm=False, output_dim=A,
                 n_gaussians=G, min_std=MIN_STD, std_activation=act, use_tanh_wrapped_distribution=False, low_noise_eval=low, device="cpu")
    g = torch.Generator().manual_seed(70 + idx)
    with torch.no_grad():      # values as after training
        for name, p in gmm.named_parameters():
            if name.endswith("weight"):
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p.shape[1]) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        gmm.std_mlp.weight.mul_(0.25)
        gmm.std_mlp.bias.sub_(0.5)      # stds around exp(-0.5): next to means of at most 0.01 and bounds near +-2 some samples reach the clamp, most do not
        gmm.logits_mlp.weight.mul_(0.6)      # logits of a standard deviation of about 2: neither uniform nor one-hot
        for p in gmm.parameters():      # on a grid of 2^-10: every value is an exact f32 (and f64), and the committed file stays small
            p.copy_(torch.round(p * 1024.0) / 1024.0)
    ag.model = SampleOnce(gmm).eval()
    ag.scaler = make_scaler(80 + idx, obs, A, spread)
    ag.min_action = torch.from_numpy(ag.scaler.y_bounds[0, :]).to(ag.device)      # bc_agent.py:106-107
    ag.max_action = torch.from_numpy(ag.scaler.y_bounds[1, :]).to(ag.device)
    return ag, gmm


class Bank:
    """Patches torch.multinomial(probs [1, G], 1, True) and torch.normal(loc, scale) [1, 1, G, A].  ``fix``: draw a fresh u per call and draw again inside EDGE of the
    row's f64 CDF (the f64 run); afterwards the bank is served as it stands (the shipped run).  The normals are banked up front."""

    def __init__(self, seed, G, A):
        self.rng = np.random.default_rng(seed)
        self.G, self.A = G, A
        self.u = np.zeros((N_ENV, T_STEPS), dtype=np.float32)
        self.z = self.rng.normal(size=(N_ENV, T_STEPS, A)).astype(np.float32)
        self.redrawn = self.calls = self.normal_calls = 0
        self.env = self.step = 0
        self.fix = True
        self.comps, self.cdf = {}, {}

    def draw(self):
        return np.float32(int(self.rng.integers(0, 1 << 24)) / float(1 << 24))

    @staticmethod
    def rule(c, u):
        return min(int((c <= float(u) * c[-1]).sum()), len(c) - 1)

    def multinomial(self, probs, num_samples=1, replacement=False, **kw):
        assert num_samples == 1 and tuple(probs.shape) == (1, self.G)
        self.calls += 1
        c = np.cumsum(probs[0].double().numpy())
        if self.fix:
            u = self.draw()
            while np.abs(float(u) * c[-1] - c).min() / c[-1] < EDGE:
                u = self.draw(); self.redrawn += 1
            self.u[self.env, self.step] = u
        u = self.u[self.env, self.step]
        key = (self.fix, self.env, self.step)
        self.comps[key], self.cdf[key] = self.rule(c, u), c / c[-1]
        return torch.full((1, 1), self.comps[key], dtype=torch.long)

    def normal(self, loc, scale, **kw):
        assert tuple(loc.shape) == tuple(scale.shape) == (1, 1, self.G, self.A)
        self.normal_calls += 1
        z = torch.from_numpy(self.z[self.env, self.step]).to(loc.dtype)
        return loc + scale * z.reshape(1, 1, 1, self.A)

    def __enter__(self):
        self._m, self._n = torch.multinomial, torch.normal
        torch.multinomial, torch.normal = self.multinomial, self.normal
        return self

    def __exit__(self, *a):
        torch.multinomial, torch.normal = self._m, self._n


def run(ag, gmm, bank, obs, f64):
    """The 24 predict calls; returns (actions [N, T, A], components [N, T], the drawn component's unclamped sample in scaled space [N, T, A]) and the dtypes seen."""
    net = gmm.mlp
    seen = []
    hook = gmm.register_forward_hook(lambda m, i, o: seen.append((i[0].detach().clone(), o)))
    keep = ag.scaler.scale_input
    bank.fix = f64
    if f64:
        gmm.double()
        sc = ag.scaler
        sc.scale_input = lambda x: (x.double().to(sc.device) - sc.x_mean) / (sc.x_std + 1e-12)
        def forward(x):      # ResidualMLPNetwork.forward without its cast to f32
            for layer in net.layers:
                x = layer(x)
            return x
        net.forward = forward
    A = bank.A
    out = (np.zeros((N_ENV, T_STEPS, A)), np.zeros((N_ENV, T_STEPS), dtype=np.int64), np.zeros((N_ENV, T_STEPS, A)))
    try:
        with bank:
            for e in range(N_ENV):
                for t in range(T_STEPS):
                    bank.env, bank.step = e, t
                    calls = (bank.calls, bank.normal_calls)
                    y = ag.predict(obs[e, t])
                    assert (bank.calls, bank.normal_calls) == (calls[0] + 1, calls[1] + 1)      # one multinomial and one normal call per sample
                    xin, dist = seen[-1]
                    assert tuple(xin.shape) == (1, 1, obs.shape[-1])
                    k = bank.comps[(f64, e, t)]
                    comp = dist.component_distribution.base_dist
                    x = comp.loc[0, 0, k] + comp.scale[0, 0, k] * torch.from_numpy(bank.z[e, t]).to(comp.loc.dtype)
                    out[0][e, t] = np.asarray(y, dtype=np.float64).reshape(-1)
                    out[1][e, t] = k
                    out[2][e, t] = x.double().numpy()
    finally:
        hook.remove()
        if f64:
            ag.scaler.scale_input = keep
            del net.forward
            gmm.float()
    return out, (xin.dtype, comp.loc.dtype, np.asarray(y).dtype)


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
    out = {}
    for idx, (name, obs_dim, A, G, hidden, layers, act, low, spread) in enumerate(CASES):
        ag, gmm = make_agent(idx, obs_dim, A, G, hidden, layers, act, low, spread)
        sd = {k: v.detach().clone() for k, v in gmm.state_dict().items()}
        lo, hi = ag.scaler.y_bounds[0].copy(), ag.scaler.y_bounds[1].copy()
        bank = Bank(90 + idx, G, A)
        rng = np.random.default_rng(100 + idx)
        obs = (ag.scaler.x_mean.numpy() + rng.normal(size=(N_ENV, T_STEPS, obs_dim)) * ag.scaler.x_std.numpy()).astype(np.float32)
        r64, dt64 = run(ag, gmm, bank, obs, True)
        r32, dt32 = run(ag, gmm, bank, obs, False)
        assert all(torch.equal(sd[k], v) for k, v in gmm.state_dict().items()) and not gmm.training
        assert np.array_equal(r32[1], r64[1]), "a component differs between the shipped and the f64 run: EDGE is too small"
        cdf_dev = max(float(np.abs(bank.cdf[(False, e, t)] - bank.cdf[(True, e, t)]).max()) for e in range(N_ENV) for t in range(T_STEPS))
        D = float(np.abs(r32[0] - r64[0]).max())
        hit = (r64[2] < lo) | (r64[2] > hi)
        cdfs = np.stack([bank.cdf[(True, e, t)] for e in range(N_ENV) for t in range(T_STEPS)])
        pmax = np.diff(np.concatenate([np.zeros((len(cdfs), 1)), cdfs], axis=1), axis=1).max(-1)
        print("case %s (obs %d, A %d, G %d, hidden %d / %d, %s, low_noise %s): dtypes of (network input, component means, returned action): shipped run %s, f64 run %s"
              % (name, obs_dim, A, G, hidden, layers, act, low, dt32, dt64))
        print("  D = %.3e (largest |action - y_mean| %.3e); max probability per row min %.3f median %.3f max %.3f; components drawn: %d distinct of %d; redrawn u: %d; "
              "EDGE %.1e, f32 CDF against f64 CDF %.3e (EDGE / 4 = %.1e); samples past a bound: %d of %d"
              % (D, float(np.abs(r64[0] - ag.scaler.y_mean.numpy()).max()), pmax.min(), np.median(pmax), pmax.max(), len(np.unique(r64[1])), r64[1].size, bank.redrawn, EDGE,
                 cdf_dev, EDGE / 4, int(hit.sum()), hit.size))
        assert cdf_dev < EDGE / 4 and D > 0
        assert len(np.unique(r64[1])) > min(G, 8) // 2 and pmax.max() < 0.999
        if name == "b":
            assert 0 < hit.sum() < hit.size      # some samples reach the clamp, not all
        # the shipped arithmetic, restated: clamp of the f32 sample against the f32 roundings of the bounds, f64 product and sum
        c32 = np.minimum(np.maximum(r32[2].astype(np.float32), lo.astype(np.float32)), hi.astype(np.float32)).astype(np.float64)
        eps = np.float64(np.float32(1e-12))      # (the scaler adds 1e-12 * torch.ones(..): an f32 tensor)
        assert np.array_equal(c32 * (ag.scaler.y_std.numpy() + eps) + ag.scaler.y_mean.numpy(), r32[0])
        pre = "gm_%s_" % name
        out.update({pre + "sd__" + k.replace(".", "__"): v.numpy() for k, v in sd.items()})
        out.update({pre + "cfg": np.array([obs_dim, A, G, hidden, layers, {"exp": 1, "softplus": 2}[act], int(low)], dtype=np.int64), pre + "min_std": np.array([MIN_STD]),
                    pre + "obs": obs, pre + "u": bank.u, pre + "z": bank.z, pre + "comps": r64[1], pre + "x_mean": ag.scaler.x_mean.numpy(), pre + "x_std": ag.scaler.x_std.numpy(),
                    pre + "y_mean": ag.scaler.y_mean.numpy(), pre + "y_std": ag.scaler.y_std.numpy(), pre + "y_bounds": ag.scaler.y_bounds, pre + "ref32": r32[0],
                    pre + "ref64": r64[0], pre + "x64": r64[2], pre + "D": np.array([D]), pre + "edge": np.array([EDGE, cdf_dev])})
    data = npz_bytes(out)
    dst = os.path.join(HERE, "ref_bc_gmm_agent.npz")
    if "--check" in sys.argv:
        same = open(dst, "rb").read() == data
        print("the committed file is reproduced byte for byte" if same else "the committed file DIFFERS from this run")
        sys.exit(0 if same else 1)
    with open(dst, "wb") as f:
        f.write(data)
    print("wrote", dst, "%.0f KB" % (len(data) / 1024))


if __name__ == "__main__":
    main()
