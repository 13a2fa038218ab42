"""Native batched policies for the rollout boundary: the reference's evaluation-time policies restated for a
BATCH of environments on device-resident observations.

The reference agents are batch-1 and numpy-in / numpy-out (``agent.predict(np.ndarray[obs]) -> np.ndarray[1, act]``,
agents/base_agent.py:110-122) with a host <-> device round trip, an EMA parameter swap (store / copy_to / restore over every
parameter) and a Python deque of the observation history inside EVERY call (ddpm_agent.py:213-274, beso_agent.py:316-443).  With the
simulator at millions of env-steps/s the policy is the bottleneck, so the classes below run the same computation once per step on
the whole batch: ``predict_batch(obs[N, obs_dim]) -> act[N, act_dim]`` with
  * the scaler (agents/utils/scaler.py:72-113) folded into two affine maps on the device,
  * the observation / action history in device ring buffers ``[N, W, dim]`` with a per-lane length (lanes that start a new
    trajectory - ``begin_episodes(mask)`` - restart their history),
  * the EMA weights swapped in ONCE (``use_ema(shadow_params)``) instead of per call,
  * the denoising loops (DDPM ancestral sampling, gc_diffusion.py:144-200; BESO Euler-ancestral on the Karras-preconditioned
    denoiser, gc_sampling.py:217-256, score_wrappers.py:20-99) running on the batch.
Networks are re-stated with the reference's parameter names, so a reference checkpoint (``model_state_dict``) loads unchanged
(``load_reference_state_dict``); tests/golden/gen_agent_goldens.py builds the reference agents with fixed-seed weights in the build
container and stores weights, inputs, noise and the reference's outputs, and tests/test_policies.py replays them here (row i of the
batch == the reference's batch-1 ``predict`` of environment i).
"""
from __future__ import annotations

import copy
import math
import os
import warnings

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F


# ------------------------------------------------------------------------------------------------ scaler
class Scaler:
    """agents/utils/scaler.py:72-113 for ``scale_data=True``: x -> (x - mean) / (std + 1e-12), y -> y (std + 1e-12) + mean."""

    def __init__(self, x_mean, x_std, y_mean, y_std, y_bounds=None, device="cuda"):
        f = lambda a: torch.as_tensor(a, dtype=torch.float32, device=device)
        self.x_mean, self.x_std, self.y_mean, self.y_std = f(x_mean), f(x_std), f(y_mean), f(y_std)
        self.y_bounds = None if y_bounds is None else f(y_bounds)

    @classmethod
    def from_reference(cls, sc, device, bounds_optional: bool = False):
        """A reference agent's scaler on ``device``; ``bounds_optional``: one without ``y_bounds`` is taken too (BeTPolicy gets its bounds from the agent)."""
        return cls(sc.x_mean, sc.x_std, sc.y_mean, sc.y_std, getattr(sc, "y_bounds", None) if bounds_optional else sc.y_bounds, device=device)

    @classmethod
    def unit(cls, obs_dim: int, action_dim: int, action_scale: float, bound: float, device):
        """The scaler of the ``random()`` policies: observations as they are, actions of ``action_scale`` per unit of the scaled space, bounds +-``bound``."""
        return cls([0.0] * obs_dim, [1.0] * obs_dim, [0.0] * action_dim, [action_scale] * action_dim, y_bounds=[[-bound] * action_dim, [bound] * action_dim], device=device)

    def scale_input(self, x):
        return ((x - self.x_mean) / (self.x_std + 1e-12)).to(torch.float32)

    def inverse_scale_output(self, y):
        return y * (self.y_std + 1e-12) + self.y_mean


# ------------------------------------------------------------------------------------------------ networks
class _ResBlock(nn.Module):          # TwoLayerPreActivationResNetLinear, agents/models/common/mlp.py:9-46 (no norm, no dropout at eval)
    def __init__(self, hidden_dim):
        super().__init__()
        self.l1, self.l2 = nn.Linear(hidden_dim, hidden_dim), nn.Linear(hidden_dim, hidden_dim)

    def forward(self, x):
        return x + self.l2(F.mish(self.l1(F.mish(x))))


class FusedResMLPHook:
    """Mixin of a module with ``_parts()`` = (lin_in, [(l1, l2), ..], lin_out): the lazily created device path (FusedResMLP, below) and its packed buffers."""

    _fused = None      # a plain attribute (no buffer, no parameter): state_dict() does not see it

    def ensure_packed(self):
        """Refresh the packed weight buffers of the device path (in place) if a parameter has changed - what a captured graph's owner calls before a replay."""
        if self._fused is not None and self._fused._fw is not None:
            self._fused.ensure_packed(self._parts())

    def invalidate_packed(self):
        """After ``param.data`` writes (invisible to the version counters): the next call / ensure_packed() repacks."""
        if self._fused is not None:
            self._fused.invalidate()

    def _fused_forward(self, x):
        """The network on x [N, in] (f32) in one launch on the f32 matrix cores, or None where the device path does not apply (D3IL_POLICY_FUSED_RESMLP=0, the
        CPU, other shapes, a caller that wants gradients): the caller then runs torch's layers."""
        if x.dim() == 2 and x.is_cuda:
            if self._fused is None:
                self._fused = FusedResMLP()
            parts = self._parts()
            if self._fused.ok(x, parts):
                return self._fused(x, parts)
        return None


class ResidualMLP(FusedResMLPHook, nn.Module):
    """ResidualMLPNetwork (agents/models/common/mlp.py:114-182), Mish: Linear, num_hidden_layers / 2 pre-activation residual blocks, Linear."""

    def __init__(self, input_dim, hidden_dim, num_hidden_layers, output_dim):
        super().__init__()
        assert num_hidden_layers % 2 == 0
        self.layers = nn.ModuleList([nn.Linear(input_dim, hidden_dim)] + [_ResBlock(hidden_dim) for _ in range(1, num_hidden_layers, 2)] + [nn.Linear(hidden_dim, output_dim)])

    def _parts(self):
        layers = list(self.layers)      # (a slice of a ModuleList builds a new ModuleList: 10 us in every eager step of the policies that ask for the parts)
        return (layers[0], [(b.l1, b.l2) for b in layers[1:-1]], layers[-1])

    @classmethod
    def from_reference_state(cls, sd, device=None):
        """The network of a reference ``ResidualMLPNetwork.state_dict()`` - widths and block count read from the keys -, loaded, on ``device`` (default: where the
        state dict lives), frozen."""
        sd = {k: torch.as_tensor(v) for k, v in sd.items()}
        hidden, in_dim = sd["layers.0.weight"].shape
        last = max(int(k.split(".")[1]) for k in sd)
        net = cls(in_dim, hidden, 2 * len({k.split(".")[1] for k in sd if ".l1." in k}), sd["layers.%d.weight" % last].shape[0])
        net.load_state_dict(sd)
        return net.to(torch.device(device) if device is not None else sd["layers.0.weight"].device).requires_grad_(False)

    @staticmethod
    def is_plain(layers, strict: bool) -> bool:
        """Are the ``layers`` of a reference ResidualMLPNetwork what this class restates: plain ``nn.Linear`` layers without spectral norm around Mish blocks without
        norm?  ``strict`` (CVAE, BeT-MLP): no subclass of nn.Linear, every layer with a bias, square blocks of the input layer's width."""
        blocks = layers[1:-1]
        lins = [layers[0], layers[-1]] + [l for b in blocks for l in (b.l1, b.l2)]
        if not all(isinstance(l, nn.Linear) and not hasattr(l, "weight_orig") for l in lins) or not all(isinstance(b.act, nn.Mish) and not b.use_norm for b in blocks):
            return False
        H = layers[0].out_features
        return not strict or (len(layers) >= 2 and all(type(l) is nn.Linear and l.bias is not None for l in lins) and layers[-1].in_features == H
                              and all(l.in_features == H and l.out_features == H for l in lins[2:]))

    @classmethod
    def random(cls, input_dim, hidden_dim, n_blocks, output_dim, seed: int, weight_gain: float = 1.0):
        """Fixed random weights for the ``random()`` policies: torch's default layer initialisation under ``seed`` (the global generator is left alone) times
        ``weight_gain``, frozen."""
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            net = cls(input_dim, hidden_dim, 2 * n_blocks, output_dim)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(weight_gain)
        return net.requires_grad_(False)

    def forward(self, x):
        x = x.to(torch.float32)
        y = self._fused_forward(x)
        if y is not None:
            return y
        for layer in self.layers:
            x = layer(x)
        return x


class _SinusoidalPosEmb(nn.Module):   # agents/models/diffusion/utils.py:9-22
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        half = self.dim // 2
        emb = torch.exp(torch.arange(half, device=x.device) * -(math.log(10000) / (half - 1)))
        emb = x[:, None] * emb[None, :]
        return torch.cat((emb.sin(), emb.cos()), dim=-1)


class DiffusionMLP(nn.Module):
    """DiffusionMLPNetwork (agents/models/diffusion/diffusion_models.py:20-118), residual style, not goal conditioned:
    eps(x, t, state) = ResidualMLP(cat(x, time_mlp(t), state))."""

    def __init__(self, action_dim, obs_dim, t_dim, hidden_dim, num_hidden_layers):
        super().__init__()
        self.temp_layers = nn.Sequential(_SinusoidalPosEmb(t_dim), nn.Linear(t_dim, t_dim * 2), nn.Mish(), nn.Linear(t_dim * 2, t_dim))
        self.layers = ResidualMLP(obs_dim + action_dim + t_dim, hidden_dim, num_hidden_layers, action_dim)

    def forward(self, x, t, state):
        t = self.temp_layers(t)
        if state.dim() == 3:
            return self.layers(torch.cat([x, t[:, None, :].expand(-1, state.shape[1], -1), state], dim=2))
        return self.layers(torch.cat([x, t, state], dim=1))


class _CausalSelfAttention(nn.Module):     # score_gpts.py:15-80
    def __init__(self, n_embd, n_heads, block_size):
        super().__init__()
        self.key, self.query, self.value, self.proj = (nn.Linear(n_embd, n_embd) for _ in range(4))
        self.register_buffer("mask", torch.tril(torch.ones(block_size, block_size)).view(1, 1, block_size, block_size))
        self.n_head = n_heads

    def forward(self, x):
        B, T, C = x.size()
        hd = C // self.n_head
        if x.is_cuda and x.dtype == torch.float32 and T <= 32 and hd <= 32:
            # device path: ONE linear layer for query | key | value, then the fused short-sequence attention kernel of the rollout
            # library (d3il_attention_causal_f32) which writes token-major output - no [B, H, T, T] tensors, no batched 11 x 20 GEMMs
            from . import capi
            w = torch.cat((self.query.weight, self.key.weight, self.value.weight), dim=0)
            bqkv = torch.cat((self.query.bias, self.key.bias, self.value.bias), dim=0)
            qkv = F.linear(x, w, bqkv).contiguous()
            y = torch.empty(B, T, C, dtype=torch.float32, device=x.device)
            capi.launch("d3il_attention_causal_f32", x.device, qkv=qkv, out=y, B=B, T=T, H=self.n_head, D=hd)
            return self.proj(y)
        k = self.key(x).view(B, T, self.n_head, hd).transpose(1, 2)
        q = self.query(x).view(B, T, self.n_head, hd).transpose(1, 2)
        v = self.value(x).view(B, T, self.n_head, hd).transpose(1, 2)
        att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(k.size(-1)))
        att = att.masked_fill(self.mask[:, :, :T, :T] == 0, float("-inf"))
        y = F.softmax(att, dim=-1) @ v
        return self.proj(y.transpose(1, 2).contiguous().view(B, T, C))


def _layer_norm(ln: nn.LayerNorm, x):
    """nn.LayerNorm; on the device the narrow-row kernel of the rollout library (the activations are [B * T][120]: torch's kernel
    reaches an eighth of the memory bandwidth on rows this short)."""
    C = x.shape[-1]
    if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and 4 <= C <= 128 and C % 4 == 0 and x.data_ptr() % 16 == 0:
        from . import capi
        y = torch.empty_like(x)
        capi.launch("d3il_layernorm_f32", x.device, x=x, weight=ln.weight, bias=ln.bias, y=y, rows=x.numel() // C, C=C, eps=float(ln.eps))
        return y
    return ln(x)


_MLP_PACK_IDX = {}


def _cached_index(build):
    """Memoise an index builder ``build(*sizes, device)`` on (its name, the sizes, the device): the indices are built on the host once and kept on the device."""
    def get(*args):
        key = (build.__name__,) + args[:-1] + (str(args[-1]),)
        if key not in _MLP_PACK_IDX:
            _MLP_PACK_IDX[key] = build(*args)
        return _MLP_PACK_IDX[key]
    get.__name__, get.__doc__ = build.__name__, build.__doc__
    return get


@_cached_index
def mlp_pack_index(C: int, H: int, device) -> torch.Tensor:
    """Gather index that puts the two weight matrices of a transformer MLP (fc1.weight [H, C], fc2.weight [C, H], flattened and concatenated, plus one
    trailing zero) into the per-chunk order d3il_mlp_gelu_residual_f32 copies to LDS: chunk c (16 hidden units) = 16 blocks of [4 g][16 i][4 e] floats (lane 16 g + i reads its float4 at [block][lane]);
    blocks q < 8: fc1.weight[16 c + i][4 (4 q + e) + g] (the A operand of step s = 4 q + e of the first product, zero for s >= C / 4); blocks 8 + t:
    fc2.weight[16 t + i][16 c + 4 g + e] (the A operand of step e of output tile t of the second product, zero for rows >= C)."""
    c = torch.arange(H // 16).view(-1, 1, 1, 1, 1)
    blk = torch.arange(8).view(1, -1, 1, 1, 1)
    g = torch.arange(4).view(1, 1, -1, 1, 1)          # lane = 16 g + i: the float4 of a lane sits at [block][lane]
    i = torch.arange(16).view(1, 1, 1, -1, 1)
    e = torch.arange(4).view(1, 1, 1, 1, -1)
    zero = C * H * 2
    s = 4 * blk + e
    i1 = torch.where(s < C // 4, (16 * c + i) * C + 4 * s + g, torch.full_like(s + c + i + g, zero))
    row = 16 * blk + i
    i2 = torch.where(row < C, C * H + row * H + 16 * c + 4 * g + e, torch.full_like(row + c + g + e, zero))
    return torch.cat((i1.expand(H // 16, 8, 4, 16, 4), i2.expand(H // 16, 8, 4, 16, 4)), dim=1).reshape(-1).to(device)


@_cached_index
def linear120_pack_index(N: int, device) -> torch.Tensor:
    """Gather index for d3il_linear120_f32: weight [N, 120] (flattened, plus one trailing zero) -> ceil(N / 16) tiles of 8 blocks of [4 g][16 i][4 e] floats,
    block q of tile t: W[16 t + i][4 (4 q + e) + g] (zero beyond N rows / 30 steps)."""
    nt = (N + 15) // 16
    t = torch.arange(nt).view(-1, 1, 1, 1, 1)
    q = torch.arange(8).view(1, -1, 1, 1, 1)
    g = torch.arange(4).view(1, 1, -1, 1, 1)
    i = torch.arange(16).view(1, 1, 1, -1, 1)
    e = torch.arange(4).view(1, 1, 1, 1, -1)
    s_, row = 4 * q + e, 16 * t + i
    idx = torch.where((s_ < 30) & (row < N), row * 120 + 4 * s_ + g, torch.full_like(row + s_ + g, N * 120))
    return idx.reshape(-1).to(device)


def pack_linear120_weights(weight: torch.Tensor) -> torch.Tensor:
    flat = torch.cat((weight.reshape(-1), weight.new_zeros(1)))
    return flat[linear120_pack_index(weight.shape[0], weight.device)]


def pack_mlp_weights(fc1: nn.Linear, fc2: nn.Linear) -> torch.Tensor:
    H, C = fc1.weight.shape
    flat = torch.cat((fc1.weight.reshape(-1), fc2.weight.reshape(-1), fc1.weight.new_zeros(1)))
    return flat[mlp_pack_index(C, H, fc1.weight.device)]


def split_f16(w: torch.Tensor):
    """(hi, lo) f16 halves of an f32 tensor as csrc/policy_f16x3.h uses them: hi = f16(w) (saturating), lo = f16((w - hi) * 2^11)."""
    w = w.detach().to(torch.float32).clamp(-65504.0, 65504.0)
    hi = w.to(torch.float16)
    lo = ((w - hi.to(torch.float32)) * 2048.0).to(torch.float16)
    return hi, lo


@_cached_index
def mlp_f16x3_pack_index(C: int, H: int, device) -> torch.Tensor:
    """Gather index [H / 32 pairs][2048 vectors][8] into cat(fc1.weight [H, C], fc2.weight [C, H], one zero) for d3il_mlp_ln_gelu_residual_f16x3 - WITHOUT the half
    dimension (the packer interleaves hi / lo): entry (c, v, e) with v < 512: tile = v // 256, s = (v // 64) % 4, lane = v % 64 -> fc1.weight[32 c + 16 tile + i][32 s + 8 g + e];
    v >= 512: t = (v - 512) // 64 -> fc2.weight[16 t + i][32 c + 16 (e >> 2) + 4 g + (e & 3)]; lane = 16 g + i; zero beyond the matrices."""
    c = torch.arange(H // 32).view(-1, 1, 1, 1, 1, 1)
    tile = torch.arange(2).view(1, -1, 1, 1, 1, 1)
    s_ = torch.arange(4).view(1, 1, -1, 1, 1, 1)
    g = torch.arange(4).view(1, 1, 1, -1, 1, 1)
    i = torch.arange(16).view(1, 1, 1, 1, -1, 1)
    e = torch.arange(8).view(1, 1, 1, 1, 1, -1)
    zero = 2 * C * H
    k = 32 * s_ + 8 * g + e
    i1 = torch.where(k < C, (32 * c + 16 * tile + i) * C + k, torch.full_like(k + c + tile + i, zero))            # [P, 2, 4, 4, 16, 8]
    t = torch.arange(8).view(1, -1, 1, 1, 1)
    c2, g2, i2_, e2 = c.view(-1, 1, 1, 1, 1), g.view(1, 1, -1, 1, 1), i.view(1, 1, 1, -1, 1), e.view(1, 1, 1, 1, -1)
    row = 16 * t + i2_
    hid = 32 * c2 + 16 * (e2 >> 2) + 4 * g2 + (e2 & 3)
    i2 = torch.where(row < C, C * H + row * H + hid, torch.full_like(row + hid, zero))                              # [P, 8, 4, 16, 8]
    P = H // 32
    return (i1.reshape(P, 512, 8).to(device), i2.reshape(P, 512, 8).to(device))


def pack_mlp_weights_f16x3(fc1_weight: torch.Tensor, fc2_weight: torch.Tensor) -> torch.Tensor:
    """f16 [H / 32 + 1 stages][2048][8]: stage k = first-product vectors ((tile * 4 + s) * 2 + p) * 64 + lane of hidden pair k (zero for the last stage), then the
    second-product vectors 1024 + (t * 2 + p) * 64 + lane of pair k - 1 (zero for stage 0); p: 0 hi, 1 lo - the software pipeline of k_mlp_gelu_residual_f16x3."""
    H, C = fc1_weight.shape
    i1, i2 = mlp_f16x3_pack_index(C, H, fc1_weight.device)
    flat = torch.cat((fc1_weight.reshape(-1), fc2_weight.reshape(-1), fc1_weight.new_zeros(1)))
    hi, lo = split_f16(flat)
    P = H // 32
    a = torch.stack((hi[i1].view(P, 8, 64, 8), lo[i1].view(P, 8, 64, 8)), dim=2).reshape(P, 1024, 8)      # [(tile, s)][p][lane]
    b = torch.stack((hi[i2].view(P, 8, 64, 8), lo[i2].view(P, 8, 64, 8)), dim=2).reshape(P, 1024, 8)      # [t][p][lane]
    z = torch.zeros_like(a[:1])
    return torch.cat((torch.cat((a, z), dim=0), torch.cat((z, b), dim=0)), dim=1).contiguous()      # [P + 1, 2048, 8]


@_cached_index
def linear120_f16x3_pack_index(N: int, C: int, device) -> torch.Tensor:
    """Gather index [2 ceil(N / 32) tiles][4 s][64 lanes][8 e] into weight [N, C] (flattened, plus one trailing zero): W[16 t + i][32 s + 8 g + e], lane = 16 g + i."""
    nt = 2 * ((N + 31) // 32)
    t = torch.arange(nt).view(-1, 1, 1, 1, 1)
    s_ = torch.arange(4).view(1, -1, 1, 1, 1)
    g = torch.arange(4).view(1, 1, -1, 1, 1)
    i = torch.arange(16).view(1, 1, 1, -1, 1)
    e = torch.arange(8).view(1, 1, 1, 1, -1)
    row, k = 16 * t + i, 32 * s_ + 8 * g + e
    return torch.where((row < N) & (k < C), row * C + k, torch.full_like(row + k, N * C)).reshape(nt, 4, 64, 8).to(device)


def pack_linear120_weights_f16x3(weight: torch.Tensor) -> torch.Tensor:
    """f16 [2 ceil(N / 32) tiles][512][8] for d3il_linear120_f16x3: vector (s * 2 + p) * 64 + lane of tile t = W_p[16 t + i][32 s + 8 g + e] (zero beyond N x 120)."""
    idx = linear120_f16x3_pack_index(*weight.shape, weight.device)
    hi, lo = split_f16(torch.cat((weight.reshape(-1), weight.new_zeros(1))))
    return torch.stack((hi[idx], lo[idx]), dim=2).reshape(idx.shape[0], 512, 8).contiguous()


def weights_out_of_range(w: torch.Tensor) -> torch.Tensor:
    """Number of entries of ``w`` that split_f16 cannot carry: NaN, +-Inf or |w| > 65504 (they saturate silently) - a 0-d int64 tensor on ``w``'s device, no
    synchronisation."""
    w = w.detach().to(torch.float32)
    return (~torch.isfinite(w) | (w.abs() > 65504.0)).sum()


_capturing = torch.cuda.is_current_stream_capturing      # is the current stream being captured into a HIP graph?  For code that already runs on the device.


def swap_in_ema(module: nn.Module, shadow_params):
    """One EMA swap per rollout (the reference swaps per predict call): shadow parameters in ``module.parameters()`` order."""
    with torch.no_grad():
        for p, sh in zip(module.parameters(), shadow_params):
            p.copy_(torch.as_tensor(sh, dtype=p.dtype, device=p.device))


class PackedWeights:
    """Packed device copies of a module's weights that follow its parameters: ``buf`` is a dict of PERSISTENT buffers, refreshed in place whenever a parameter has
    changed (tensor version counters: no device synchronisation).  The addresses never change while names, shapes, dtypes and devices stay, so a captured HIP graph
    keeps reading the current weights as long as ``ensure`` runs before every replay - e.g. after the EMA swap of a rollout.  The parameters and the pack function
    come with every call (no reference to the module is kept): a deep copy of the module gets its own buffers and packs ITS weights into them."""

    def __init__(self):
        self.buf, self.key = None, None

    def invalidate(self):
        """Force a repack at the next ensure().  Needed after writes that bypass the tensors' version counters - ``param.data.copy_(...)`` as the reference's EMA
        helper does in copy_to / restore (agents/models/.../ema.py); ``use_ema()``, ``load_state_dict`` and in-place ops on the parameters are seen without it."""
        self.key = None

    def ensure(self, params, pack):
        """``pack() -> {name: tensor or plain value}`` runs only when the (data_ptr, _version) key of ``params`` has changed."""
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self.key == key:
            return
        with torch.no_grad():
            new, old = pack(), self.buf
        layout = lambda d: {k: (v.shape, v.dtype, v.device) if torch.is_tensor(v) else None for k, v in d.items()}
        if old is not None and layout(old) == layout(new):
            for k, v in new.items():
                if torch.is_tensor(v):
                    old[k].copy_(v)
                else:
                    old[k] = v
        else:
            # first pack, another layout or another device (the module has moved): new buffers, the cache's OWN (a pack function may hand back a view of a parameter,
            # e.g. an f32 bias as it is: refreshing that in place would write the parameter and bump the very version counter the key is made of)
            self.buf = {k: v.clone() if torch.is_tensor(v) else v for k, v in new.items()}
        self.key = key

    def current(self, params, pack):
        """The buffers for a launch: refreshed here, except inside a graph capture, where packing kernels must not be recorded - they have to be packed already."""
        if _capturing():
            assert self.key is not None, "a captured graph replays the packed weight buffers: call ensure_packed() before capturing"
        else:
            self.ensure(params, pack)
        return self.buf


# ------------------------------------------------------------------------------------------------ range / NaN guard of the split-f16 kernels
_RANGE_GUARD = None          # the guard whose counters the library currently writes (d3il_f16x3_set_guard), or None
_GUARD_EPOCH = 0             # bumped by every enable / disable: a graph captured under another epoch launches the wrong instantiation and is captured again
_ENV_GUARD_TRIED = False


class RangeGuard:
    """Owner of the device int64[4] the guarded split-f16 kernels count into (include/d3il_rollout.h d3il_f16x3_set_guard): rows with an operand beyond +-65504
    (``clipped``; they saturate as without the guard), rows with a NaN / Inf operand (``nonfinite``; they come out NaN instead of finite) and ``launches``.
    One guard is active per process (the module keeps it alive while the library holds its address); ``with RangeGuard(dev) as g: ...; g.read()``.  Counts are per launch: a NaN row is counted again by every kernel it passes."""

    def __init__(self, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("RangeGuard counts inside the split-f16 HIP kernels: it needs a HIP device (got %s, device available: %s)" % (dev, torch.cuda.is_available()))
        self.counts = torch.zeros(4, dtype=torch.int64, device=dev)
        self.enabled = False

    def enable(self):
        global _RANGE_GUARD, _GUARD_EPOCH
        from . import capi
        if _RANGE_GUARD is not None and _RANGE_GUARD is not self:
            _RANGE_GUARD.enabled = False
        capi.check(capi.load().d3il_f16x3_set_guard(self.counts.data_ptr()))
        _RANGE_GUARD, self.enabled = self, True
        _GUARD_EPOCH += 1
        return self

    def disable(self):
        global _RANGE_GUARD, _GUARD_EPOCH
        if _RANGE_GUARD is self:
            from . import capi
            torch.cuda.synchronize(self.counts.device)      # launches in flight still write the counters
            capi.check(capi.load().d3il_f16x3_set_guard(None))
            _RANGE_GUARD = None
            _GUARD_EPOCH += 1
        self.enabled = False

    def reset(self):
        self.counts.zero_()

    def read(self) -> dict:
        torch.cuda.synchronize(self.counts.device)      # every stream of the device: sub-batches launch the policy kernels on streams of their own
        c = self.counts.tolist()
        return {"clipped": c[0], "nonfinite": c[1], "launches": c[2]}

    def __enter__(self):
        return self.enable()

    def __exit__(self, *exc):
        self.disable()
        return False


def range_guard():
    """The process's active RangeGuard, or None."""
    return _RANGE_GUARD


def guard_epoch() -> int:
    return _GUARD_EPOCH


def _env_range_guard(device):
    """D3IL_POLICY_RANGE_GUARD=1: create and enable a guard at the first f16x3 call of the process (outside a graph capture)."""
    global _ENV_GUARD_TRIED
    if _ENV_GUARD_TRIED or _capturing():
        return
    _ENV_GUARD_TRIED = True
    if os.environ.get("D3IL_POLICY_RANGE_GUARD", "0") == "1" and _RANGE_GUARD is None:
        RangeGuard(device).enable()


def policy_gemm_mode() -> str:
    """Which matrix-core path the DiffusionGPT blocks take: "f16x3" (default: split-f16 products, csrc/policy_f16x3.h) or "f32" (D3IL_POLICY_GEMM=f32: the f32-input MFMA
    kernels of rounds 3 - 5)."""
    return os.environ.get("D3IL_POLICY_GEMM", "f16x3")


class _Block(nn.Module):                   # score_gpts.py:83-115
    def __init__(self, n_embd, n_heads, block_size):
        super().__init__()
        self.ln1, self.ln2 = nn.LayerNorm(n_embd), nn.LayerNorm(n_embd)
        self.attn = _CausalSelfAttention(n_embd, n_heads, block_size)
        self.mlp = nn.Sequential(nn.Linear(n_embd, 4 * n_embd), nn.GELU(), nn.Linear(4 * n_embd, n_embd), nn.Dropout(0.0))
        self._packed = PackedWeights()      # a plain attribute: state_dict() keeps the reference's names

    def _fused_static_ok(self):
        return (self.mlp[0].weight.shape == (480, 120) and self.mlp[0].weight.is_cuda and self.mlp[0].weight.dtype == torch.float32 and 120 // self.attn.n_head <= 32
                and os.environ.get("D3IL_POLICY_FUSED_MLP", "1") == "1")

    def _fused_ok(self, x):
        # the matrix-core kernels are inference only (no autograd node): any caller that wants gradients - fine-tuning, a gradient check - takes the torch path
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return self._fused_static_ok() and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] == 120 and x.data_ptr() % 16 == 0 and x.shape[1] <= 32

    def invalidate_packed(self):
        """Force a repack at the next ensure_packed() (after ``param.data`` writes, which the version counters do not see)."""
        self._packed.invalidate()

    def _pack_params(self):
        a = self.attn
        return (a.query.weight, a.key.weight, a.value.weight, a.query.bias, a.key.bias, a.value.bias, a.proj.weight, self.mlp[0].weight, self.mlp[2].weight)

    def _pack(self):
        """The block's weights in the tile order of the matrix-core kernels: ``wp_*`` for the f32-input kernels, ``hp_*`` the split-f16 forms of the same three
        matrices (csrc/policy_f16x3.h)."""
        a, fc1, fc2 = self.attn, self.mlp[0], self.mlp[2]
        wq = torch.cat((a.query.weight, a.key.weight, a.value.weight), dim=0)
        hp_qkv, hp_proj = pack_linear120_weights_f16x3(wq), pack_linear120_weights_f16x3(a.proj.weight)
        return {"wp_qkv": pack_linear120_weights(wq), "wp_proj": pack_linear120_weights(a.proj.weight), "wp_mlp": pack_mlp_weights(fc1, fc2),
                "b_qkv": torch.cat((a.query.bias, a.key.bias, a.value.bias), dim=0),
                "hp_qkv": hp_qkv, "hp_proj": hp_proj, "hp_mlp": pack_mlp_weights_f16x3(fc1.weight, fc2.weight),
                # (query | key | value) tiles followed by the projection's: the weight stream of the one-kernel attention half (d3il_attn_half_f16x3)
                "hp_attn": torch.cat((hp_qkv, hp_proj), dim=0),
                # entries of the f16x3-packed matrices that the split cannot carry (device scalar, no synchronisation; BESOPolicy.range_report)
                "w_oor": weights_out_of_range(wq) + weights_out_of_range(a.proj.weight) + weights_out_of_range(fc1.weight) + weights_out_of_range(fc2.weight)}

    def ensure_packed(self):
        """Refresh the packed weights (PackedWeights: in place while the module stays on its device) - BESOPolicy.predict_batch does before every replay."""
        self._packed.ensure(self._pack_params(), self._pack)

    def forward(self, x, keep=None):
        """keep: token positions (LongTensor) whose outputs are needed; the block then returns [B, len(keep), C] - attention still sees every token, the output
        projection and the MLP run on the kept rows only (the last block of DiffusionGPT: only the action positions are decoded)."""
        if self._fused_ok(x):
            # device path, four kernels of the rollout library per block, all GEMMs on the matrix cores (split-f16 products by default, policy_gemm_mode()) with the
            # LayerNorms, biases, GELU and residuals fused in: ln1 + (query | key | value) product -> causal attention -> output projection + residual -> ln2 + fc1 + GELU + fc2 + residual
            # (the [B T][480] hidden activations stay in registers)
            from . import capi
            dev = x.device
            B, T, C = x.shape
            M = B * T
            a = self.attn
            w = self._packed.current(self._pack_params(), self._pack)
            f16x3 = policy_gemm_mode() == "f16x3"
            if f16x3 and not _ENV_GUARD_TRIED:
                _env_range_guard(dev)
            linear, mlp = ("d3il_linear120_f16x3", "d3il_mlp_ln_gelu_residual_f16x3") if f16x3 else ("d3il_linear120_f32", "d3il_mlp_ln_gelu_residual_f32")
            w_qkv, w_proj, w_mlp = (w["hp_qkv"], w["hp_proj"], w["hp_mlp"]) if f16x3 else (w["wp_qkv"], w["wp_proj"], w["wp_mlp"])
            ln1 = dict(ln_weight=self.ln1.weight, ln_bias=self.ln1.bias, ln_eps=float(self.ln1.eps))
            if f16x3 and T <= 16 and a.n_head == 6 and w["hp_attn"].shape[0] == 32 and os.environ.get("D3IL_POLICY_FUSED_ATTN", "1") == "1":
                # the attention half in ONE launch, one wave per sequence: q | k | v and the attention output never leave the CU (csrc/policy_f16x3.h k_attn_half_f16x3)
                x1 = torch.empty_like(x)
                capi.launch("d3il_attn_half_f16x3", dev, x=x, **ln1, w_packed=w["hp_attn"], b_qkv=w["b_qkv"], b_proj=a.proj.bias, out=x1, n_seq=B, T=T, n_head=a.n_head, C=C)
                if keep is not None:
                    x1 = x1.index_select(1, keep)
                    M = x1.shape[0] * x1.shape[1]
            else:
                qkv = torch.empty(B, T, 3 * C, dtype=torch.float32, device=dev)
                capi.launch(linear, dev, xin=x, **ln1, w_packed=w_qkv, bias=w["b_qkv"], resid=None, out=qkv, rows=M, N=3 * C)
                y = torch.empty_like(x)
                capi.launch("d3il_attention_causal_f32", dev, qkv=qkv, out=y, B=B, T=T, H=a.n_head, D=C // a.n_head)
                if keep is not None:
                    y, x = y.index_select(1, keep), x.index_select(1, keep)
                    M = y.shape[0] * y.shape[1]
                x1 = torch.empty_like(x)
                capi.launch(linear, dev, xin=y, ln_weight=None, ln_bias=None, ln_eps=0.0, w_packed=w_proj, bias=a.proj.bias, resid=x, out=x1, rows=M, N=C)
            out = torch.empty_like(x1)
            capi.launch(mlp, dev, h=x1, ln_weight=self.ln2.weight, ln_bias=self.ln2.bias, ln_eps=float(self.ln2.eps), x=x1, w_packed=w_mlp, b1=self.mlp[0].bias,
                        b2=self.mlp[2].bias, out=out, rows=M, C=120, H=480)
            return out
        x = x + self.attn(_layer_norm(self.ln1, x))
        if keep is not None:
            x = x.index_select(1, keep)
        return x + self.mlp(_layer_norm(self.ln2, x))


for _name in ("wp_qkv", "wp_proj", "wp_mlp", "b_qkv", "hp_qkv", "hp_proj", "hp_mlp", "hp_attn", "w_oor"):      # the packed tensors under their earlier names, read-only
    setattr(_Block, "_" + _name, property(lambda self, _name=_name: self._packed.buf[_name]))


# ------------------------------------------------------------------------------------------------ the 72-wide trunk: the whole block chain in one launch
TRUNK72_STAGES, TRUNK72_STAGE_V, TRUNK72_VEC = 28, 768, 936      # csrc/policy_trunk72.h: stages per layer, 16-byte vectors per stage, f32 vector entries per layer
TRUNK72_WIDE_TILES = 2048      # (T72_WIDE_TILES: launches of that many 16-row tiles use workgroups of eight tiles, smaller ones of four)
TRUNK72_DEFAULT = "1"          # D3IL_POLICY_TRUNK72 when unset (what the measurement chose)


@_cached_index
def trunk72_pack_index(device) -> torch.Tensor:
    """Gather index [28 stages][6][64 lanes][8 e] into cat(Wqkv [216, 72], Wproj [72, 72], W1 [288, 72], W2 [72, 288], one zero) of ONE layer for
    d3il_gpt_trunk72_f16x3 - without the half dimension (the packer interleaves hi / lo), lane = 16 g + i:
    stages 0 .. 6 (q | k | v) and 7 .. 9 (projection): entry (u * 3 + s) = W[16 (2 stage + u) + i][32 s + 8 g + e]; stage 10 + 2 k: the same form with fc1's tiles 2 k + u;
    stage 11 + 2 k: entry t = W2[16 t + i][32 k + 16 (e >> 2) + 4 g + (e & 3)]; zero beyond the matrices."""
    C, H = 72, 288
    bases = (0, 3 * C * C, 4 * C * C, 4 * C * C + H * C)
    zero = 4 * C * C + 2 * H * C
    s_ = torch.arange(3).view(1, -1, 1, 1, 1)
    g = torch.arange(4).view(1, 1, -1, 1, 1)
    i = torch.arange(16).view(1, 1, 1, -1, 1)
    e = torch.arange(8).view(1, 1, 1, 1, -1)

    def product(n_tiles, N, base):      # [n_tiles / 2 stages][6 = (u, s)][64][8]
        t = torch.arange(n_tiles).view(-1, 1, 1, 1, 1)
        row, k = 16 * t + i, 32 * s_ + 8 * g + e
        return torch.where((row < N) & (k < C), base + row * C + k, torch.full_like(row + k, zero)).reshape(n_tiles // 2, 6, 64, 8)

    k_ = torch.arange(H // 32).view(-1, 1, 1, 1, 1)
    t6 = torch.arange(6).view(1, -1, 1, 1, 1)
    row, hid = 16 * t6 + i, 32 * k_ + 16 * (e >> 2) + 4 * g + (e & 3)
    fc2 = torch.where(row < C, bases[3] + row * H + hid, torch.full_like(row + hid, zero)).reshape(H // 32, 6, 64, 8)
    mlp = torch.stack((product(H // 16, H, bases[2]), fc2), dim=1).reshape(2 * (H // 32), 6, 64, 8)
    idx = torch.cat((product(14, 3 * C, bases[0]), product(6, C, bases[1]), mlp), dim=0)
    assert idx.shape[0] == TRUNK72_STAGES
    return idx.to(device)


def trunk72_layer_matrices(blk):
    """The four matrices of a block in the order trunk72_pack_index reads them: Wqkv (query | key | value rows), Wproj, W1, W2."""
    a = blk.attn
    return (torch.cat((a.query.weight, a.key.weight, a.value.weight), dim=0), a.proj.weight, blk.mlp[0].weight, blk.mlp[2].weight)


def pack_trunk72_weights(blocks) -> dict:
    """The chain's weights for d3il_gpt_trunk72_f16x3: ``w`` f16 [n_layer][28][768][8] (vector (entry * 2 + p) * 64 + lane of a stage: p = 0 the high half, 1 the low half
    times 2^11; the layout is in include/d3il_rollout.h), ``vec`` f32 [n_layer][936] = ln1.w | ln1.b | b_qkv | b_proj | ln2.w | ln2.b | b1 | b2, ``w_oor`` the entries
    of the matrices the split cannot carry (0-d int64, no synchronisation)."""
    ws, vecs, oor = [], [], 0
    for blk in blocks:
        mats = trunk72_layer_matrices(blk)
        idx = trunk72_pack_index(mats[0].device)
        hi, lo = split_f16(torch.cat([m.reshape(-1) for m in mats] + [mats[0].new_zeros(1)]))
        ws.append(torch.stack((hi[idx], lo[idx]), dim=2).reshape(TRUNK72_STAGES, TRUNK72_STAGE_V, 8))
        a = blk.attn
        vecs.append(torch.cat((blk.ln1.weight, blk.ln1.bias, a.query.bias, a.key.bias, a.value.bias, a.proj.bias, blk.ln2.weight, blk.ln2.bias, blk.mlp[0].bias,
                               blk.mlp[2].bias)).detach().to(torch.float32))
        oor = oor + sum(weights_out_of_range(m) for m in mats)
    return {"w": torch.stack(ws).contiguous(), "vec": torch.stack(vecs).contiguous(), "w_oor": oor}


def _trunk72_params(blocks):
    out = []
    for blk in blocks:
        a = blk.attn
        out += [a.query.weight, a.key.weight, a.value.weight, a.proj.weight, blk.mlp[0].weight, blk.mlp[2].weight, blk.ln1.weight, blk.ln1.bias, a.query.bias, a.key.bias,
                a.value.bias, a.proj.bias, blk.ln2.weight, blk.ln2.bias, blk.mlp[0].bias, blk.mlp[2].bias]
    return out


def trunk72_packed(blocks) -> PackedWeights:
    """The chain's PackedWeights, a plain attribute of the ``nn.Sequential`` of blocks (state_dict() keeps the reference's names; a deep copy gets its own)."""
    pw = blocks.__dict__.get("_trunk72")
    if pw is None:
        pw = blocks.__dict__["_trunk72"] = PackedWeights()
    return pw


def trunk72_shape_refusal(blocks):
    """Why the chain ``blocks`` is not the shape d3il_gpt_trunk72_f16x3 is built for (n_embd 72 in 4 heads, hidden 288, 1 .. 8 blocks, ONE LayerNorm epsilon), or None."""
    if not isinstance(blocks, nn.Sequential) or not 1 <= len(blocks) <= 8:
        return "needs 1 .. 8 blocks in an nn.Sequential"
    for blk in blocks:
        if not isinstance(blk, _Block) or tuple(blk.mlp[0].weight.shape) != (288, 72) or tuple(blk.mlp[2].weight.shape) != (72, 288) or blk.attn.n_head != 4:
            return "a block is not (n_embd 72, 4 heads, hidden 288)"
        if blk.ln1.eps != blocks[0].ln1.eps or blk.ln2.eps != blocks[0].ln1.eps:
            return "the LayerNorms differ in eps"
    return None


def trunk72_switch_on() -> bool:
    return policy_gemm_mode() == "f16x3" and os.environ.get("D3IL_POLICY_TRUNK72", TRUNK72_DEFAULT) != "0"


def trunk72_static_ok(blocks) -> bool:
    """The chain takes the one-launch trunk kernel wherever its input allows: shape, f32 on a HIP device, D3IL_POLICY_GEMM=f16x3 and D3IL_POLICY_TRUNK72 not 0."""
    if not trunk72_switch_on() or trunk72_shape_refusal(blocks) is not None:      # (the switch first: two dictionary reads when it is off)
        return False
    return all(blk.mlp[0].weight.is_cuda and blk.mlp[0].weight.dtype == torch.float32 for blk in blocks)


def trunk72_input_refusal(blocks, x):
    """Why the input ``x`` cannot go through the trunk kernel (whatever the device), or None: contiguous f32 [B >= 1, T <= 16, 72], 16-byte aligned, no gradients wanted."""
    if x.dim() != 3 or x.shape[2] != 72 or not 1 <= x.shape[1] <= 16 or x.shape[0] < 1:
        return "x is not [B >= 1, 1 <= T <= 16, 72]"
    if x.dtype != torch.float32 or not x.is_contiguous() or x.data_ptr() % 16 != 0:
        return "x is not contiguous, 16-byte aligned f32"
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in blocks.parameters())):
        return "gradients are wanted (the kernel is inference only)"
    return None


def trunk72(blocks, x):
    """The block chain on x [B, T, 72] through d3il_gpt_trunk72_f16x3 (the caller has checked trunk72_static_ok / trunk72_input_refusal)."""
    from . import capi
    if not _ENV_GUARD_TRIED:
        _env_range_guard(x.device)
    w = trunk72_packed(blocks).current(_trunk72_params(blocks), lambda: pack_trunk72_weights(blocks))
    out = torch.empty_like(x)
    capi.launch("d3il_gpt_trunk72_f16x3", x.device, x=x, w_packed=w["w"], vec=w["vec"], ln_eps=float(blocks[0].ln1.eps), out=out, n_seq=x.shape[0], T=x.shape[1],
                n_layer=len(blocks))
    return out


def run_blocks(blocks, x, keep=None):
    """The one place that walks a block chain: ``blocks`` (the nn.Sequential of _Block) on x [B, T, C]; with ``keep`` (token positions) the result is [B, len(keep), C].
    A 72-wide chain of 4-head blocks on a HIP device runs as ONE launch (trunk72) and the rows are selected afterwards - everything behind the attention is row-wise,
    the numbers are the same; every other chain runs block by block, the last one with ``keep``."""
    if x.is_cuda and trunk72_static_ok(blocks) and trunk72_input_refusal(blocks, x) is None:
        out = trunk72(blocks, x)
        return out if keep is None else out.index_select(1, keep)
    for blk in blocks[:-1]:
        x = blk(x)
    return blocks[-1](x, keep=keep)


def ensure_blocks_packed(blocks) -> list:
    """ensure_packed() of every block that can take the matrix-core kernels, and of the chain's own pack where it takes the trunk kernel (OUTSIDE a captured chain:
    an EMA swap changes the packed copies); returns those blocks."""
    fused = [blk for blk in blocks if blk._fused_static_ok()]
    for blk in fused:
        blk.ensure_packed()
    if trunk72_static_ok(blocks):
        trunk72_packed(blocks).ensure(_trunk72_params(blocks), lambda: pack_trunk72_weights(blocks))
    return fused


def invalidate_blocks_packed(blocks):
    """Force a repack of the blocks' and the chain's packed weights at the next ensure (after ``param.data`` writes, which the version counters do not see)."""
    for blk in blocks:
        blk.invalidate_packed()
    if isinstance(blocks, nn.Module) and "_trunk72" in blocks.__dict__:
        blocks.__dict__["_trunk72"].invalidate()


def blocks_f16x3(blocks) -> bool:
    """Does the chain run split-f16 kernels the range guard instruments (the blocks' own or the trunk kernel)?"""
    return policy_gemm_mode() == "f16x3" and (any(blk._fused_static_ok() for blk in blocks) or trunk72_static_ok(blocks))


def blocks_w_oor(blocks) -> int:
    """Entries of the chain's f16x3-packed matrices that are NaN / Inf or beyond +-65504 (packing first where needed); one synchronising read."""
    n = sum(blk._w_oor for blk in ensure_blocks_packed(blocks))
    if trunk72_static_ok(blocks):
        n = n + trunk72_packed(blocks).buf["w_oor"]
    return int(n)


class DiffusionGPT(nn.Module):
    """DiffusionGPT (score_gpts.py:118-361), not goal conditioned: tokens = [sigma, s_1, a_1, ..., s_t, a_t], causal transformer,
    the action positions are decoded."""

    def __init__(self, state_dim, action_dim, embed_dim, n_layers, n_heads, obs_seq_len, linear_output=True):
        super().__init__()
        block_size = 2 * obs_seq_len + 1
        self.tok_emb = nn.Linear(state_dim, embed_dim)
        self.pos_emb = nn.Parameter(torch.zeros(1, obs_seq_len + 1, embed_dim))
        self.blocks = nn.Sequential(*[_Block(embed_dim, n_heads, block_size) for _ in range(n_layers)])
        self.ln_f = nn.LayerNorm(embed_dim)
        self.sigma_emb = nn.Linear(1, embed_dim)
        self.action_emb = nn.Linear(action_dim, embed_dim)
        self.action_pred = nn.Linear(embed_dim, action_dim) if linear_output else nn.Sequential(nn.Linear(embed_dim, 100), nn.SiLU(), nn.Linear(100, action_dim))
        self.obs_seq_len, self.embed_dim = obs_seq_len, embed_dim

    # ---- the sampling loop's form (BESOPolicy._sample on the device): everything that does not change between the sampling steps of one predict call is computed
    # once (state tokens, position rows, the sigma embeddings of the whole schedule), the token buffer [b, 2 t + 1, C] is filled in place - 3 small kernels per
    # step in front of the blocks instead of ~12 (mul, 2 linear, 2 add, log, div, full, stack, permute copy, cat)
    def begin_sampling(self, states, sigmas):
        b, t, _ = states.size()
        C = self.embed_dim
        pos = self.pos_emb[0, :t, :]
        xbuf = torch.empty(b, 2 * t + 1, C, dtype=torch.float32, device=states.device)
        torch.add(self.tok_emb(states), pos, out=xbuf[:, 1::2])                              # state tokens: the same in every sampling step
        emb_all = self.sigma_emb(sigmas.reshape(-1, 1).log() / 4)                                # [steps, C]; sigmas: a DEVICE tensor (no host copy inside a captured loop)
        bias_pos = (self.action_emb.bias + pos).repeat(b, 1)                                  # [b t, C]: action_emb's bias + position rows
        return dict(xbuf=xbuf, emb_all=emb_all, bias_pos=bias_pos, keep=torch.arange(2, 2 * t + 1, 2, device=states.device), t=t, b=b)

    def forward_step(self, ctx, actions, i: int, c_in: float):
        """The network on (states of begin_sampling, c_in * actions, sigma_i): same numbers as forward() up to f32 rounding of c_in (W a) against W (c_in a)."""
        b, t, xbuf = ctx["b"], ctx["t"], ctx["xbuf"]
        xbuf[:, 0] = ctx["emb_all"][i]
        xbuf[:, 2::2] = torch.addmm(ctx["bias_pos"], actions.reshape(b * t, -1), self.action_emb.weight.t(), alpha=c_in).view(b, t, -1)
        x = _layer_norm(self.ln_f, run_blocks(self.blocks, xbuf, keep=ctx["keep"]).contiguous())
        return self.action_pred(x)

    def hidden(self, xbuf, keep):
        """The block chain on a token buffer [b, 2 t + 1, C]: the last block's output at the positions ``keep`` (before ln_f) - BESONativePolicy's form."""
        return run_blocks(self.blocks, xbuf, keep=keep)

    def forward(self, states, actions, sigma):
        b, t, _ = states.size()
        emb_t = self.sigma_emb((sigma.log() / 4).reshape(b, 1).to(torch.float32)).unsqueeze(1)
        pos = self.pos_emb[:, :t, :]
        state_x, action_x = self.tok_emb(states) + pos, self.action_emb(actions) + pos
        sa = torch.stack([state_x, action_x], dim=1).permute(0, 2, 1, 3).reshape(b, 2 * t, self.embed_dim)
        x = torch.cat([emb_t, sa], dim=1)
        # only the action positions (tokens 2, 4, ..., 2 t) are decoded: the last block's output projection and MLP, the final LayerNorm and the head run
        # on those rows only (row-wise operations: the same numbers as decoding everything and slicing, score_gpts.py:340-361)
        keep = torch.arange(2, 2 * t + 1, 2, device=x.device)
        x = _layer_norm(self.ln_f, run_blocks(self.blocks, x, keep=keep).contiguous())
        return self.action_pred(x)


# ------------------------------------------------------------------------------------------------ history ring buffer
class _History:
    """Device ring buffer [N, W, dim], newest entry last, with a per-lane length: the deque(maxlen=W) of the reference agents for a
    batch.  Lanes are grouped by length for the network call (all lanes run in lock step unless some restart their trajectory)."""

    def __init__(self, n, w, dim, device):
        self.buf = torch.zeros(n, w, dim, dtype=torch.float32, device=device)
        self.len = torch.zeros(n, dtype=torch.int64, device=device)
        self.w = w
        self.lockstep = 0           # host copy of the common length, or -1 when lanes differ

    def reset(self, mask=None):
        if mask is None:
            self.len.zero_(); self.lockstep = 0
        else:
            self.len = torch.where(mask.bool(), torch.zeros_like(self.len), self.len)
            self.lockstep = -1

    def append(self, x):
        self.buf = torch.cat((self.buf[:, 1:], x.unsqueeze(1)), dim=1)
        self.len = (self.len + 1).clamp_max(self.w)
        if self.lockstep >= 0:
            self.lockstep = min(self.lockstep + 1, self.w)

    def append_(self, x):
        """append() written INTO the buffers (no new tensors: a captured graph that holds their addresses keeps working on the live history)."""
        self.buf[:, :-1] = self.buf[:, 1:].clone()
        self.buf[:, -1] = x
        self.len.add_(1).clamp_(max=self.w)
        if self.lockstep >= 0:
            self.lockstep = min(self.lockstep + 1, self.w)

    def reset_(self, mask):
        """reset(mask) in place."""
        self.len.masked_fill_(mask.to(self.len.device).bool().reshape(-1), 0)
        self.lockstep = -1

    def snapshot(self):
        return self.buf.clone(), self.len.clone(), self.lockstep

    def restore(self, snap):
        """Put a snapshot back INTO the buffers (a captured graph holds their addresses)."""
        buf, ln, self.lockstep = snap
        self.buf.copy_(buf); self.len.copy_(ln)

    def copy(self):
        c = copy.copy(self)
        c.buf, c.len = self.buf.clone(), self.len.clone()
        return c

    def padded(self):
        """Lanes with different history lengths in ONE batch: (window [N, W, dim], lengths [N]) with every lane's entries left-aligned, oldest first, and zeros on
        the right up to the window size.  A causal network whose position embedding counts from the first token never lets a lane's tokens see the padding behind
        them; the newest entry of lane i sits at position len_i - 1."""
        W, L = self.w, self.len
        j = torch.arange(W, device=self.buf.device)
        src = ((W - L).unsqueeze(1) + j).clamp_max(W - 1)
        return torch.gather(self.buf, 1, src.unsqueeze(2).expand(-1, -1, self.buf.shape[2])) * (j < L.unsqueeze(1)).unsqueeze(2), L

    def groups(self):
        """[(L, lane index tensor or None for all lanes)] - one entry when the lanes are in lock step."""
        if self.lockstep >= 0:
            return [(self.lockstep, None)]
        lens = torch.unique(self.len).tolist()          # host sync, only while lanes differ
        if len(lens) == 1:
            self.lockstep = int(lens[0])
            return [(self.lockstep, None)]
        return [(int(L), torch.nonzero(self.len == L).reshape(-1)) for L in lens]


# ------------------------------------------------------------------------------------------------ policies
class BCPolicy:
    """BC_Agent.predict (agents/bc_agent.py:240-271) on a batch: scale, MLP, clamp to the data bounds, inverse scale."""

    def __init__(self, model: ResidualMLP, scaler: Scaler, min_action, max_action):
        self.model, self.scaler = model.eval(), scaler
        dev = scaler.x_mean.device
        self.min_action, self.max_action = torch.as_tensor(min_action, device=dev), torch.as_tensor(max_action, device=dev)

    def reset(self):
        pass

    def ensure_packed(self):
        self.model.ensure_packed()

    @torch.no_grad()
    def predict_batch(self, obs):
        out = self.model(self.scaler.scale_input(obs.to(torch.float32)))
        return self.scaler.inverse_scale_output(torch.clamp(out, self.min_action, self.max_action))


def pack_resmlp_weights(lin_in, blocks, lin_out, in_cols: int = 32) -> dict:
    """Linear, residual blocks [(l1, l2), ..], Linear of a ResidualMLPNetwork in the operand order of k_resmlp_f32 and k_ddpm_mlp_f32, for any hidden
    width that is a multiple of 16: [T_out][t][lane (g, i)][r] = W[16 T_out + i][16 t + 4 g + r] for the square layers and the output layer (rows and bias padded
    to 16 with zeros; k_ddpm_mlp_f32 reads two of them); the input layer, columns padded to ``in_cols`` (32; 64 for k_cvae_decode): [T_out][lane (g, i)][s] =
    W[16 T_out + i][4 s + g], s < in_cols / 4."""
    dev = lin_in.weight.device
    H = lin_in.out_features
    NT = H // 16
    ar = lambda k: torch.arange(k, device=dev)
    To, t, g, i, r = ar(NT)[:, None, None, None, None], ar(NT)[None, :, None, None, None], ar(4)[None, None, :, None, None], ar(16)[None, None, None, :, None], ar(4)[None, None, None, None, :]
    pack = lambda W: W[16 * To + i, 16 * t + 4 * g + r].reshape(NT, NT, 64, 4)
    assert in_cols % 4 == 0 and lin_in.in_features <= in_cols
    wi = torch.zeros(H, in_cols, device=dev)
    wi[:, :lin_in.in_features] = lin_in.weight
    w_in = wi[16 * ar(NT)[:, None, None, None] + ar(16)[None, None, :, None], 4 * ar(in_cols // 4)[None, None, None, :] + ar(4)[None, :, None, None]].reshape(NT, 64, in_cols // 4)
    wo = torch.zeros(16, H, device=dev)
    wo[:lin_out.out_features] = lin_out.weight
    w_out = wo[i[0], 16 * t[0] + 4 * g[0] + r[0]].reshape(NT, 64, 4)
    bo = torch.zeros(16, device=dev)
    bo[:lin_out.out_features] = lin_out.bias
    if blocks:
        w_blk = torch.stack([pack(l.weight) for b in blocks for l in b])
        b_blk = torch.stack([l.bias for b in blocks for l in b])
    else:
        w_blk, b_blk = torch.zeros(1, NT, NT, 64, 4, device=dev), torch.zeros(1, H, device=dev)
    f = lambda x: x.detach().to(torch.float32).contiguous()
    return {"w_in": f(w_in), "b_in": f(lin_in.bias), "w_blk": f(w_blk), "b_blk": f(b_blk), "w_out": f(w_out), "b_out": f(bo), "n_blocks": len(blocks)}


def resmlp_args(w) -> dict:
    """The packed input layer and blocks under the parameter names the kernel entries give them (include/d3il_rollout.h)."""
    return dict(w_in=w["w_in"], b_in=w["b_in"], w_blocks=w["w_blk"], b_blocks=w["b_blk"])


class FusedResMLP:
    """The device path of a ResidualMLPNetwork (csrc/policy_resmlp.h k_resmlp_f32 through d3il_resmlp_f32) on packed weights (PackedWeights).  Every call takes
    ``parts`` = (lin_in, [(l1, l2), ..], lin_out) of the module it serves (no reference to the module is kept).  Non-finite input: a row of x with a NaN / Inf comes
    out NaN in every column, as from torch's layers, and no other row changes (tests/test_gpu_policy_f32_edges.py)."""

    def __init__(self):
        self._packed = PackedWeights()

    _fw, _key = property(lambda self: self._packed.buf), property(lambda self: self._packed.key)      # read-only views of the cache

    def invalidate(self):
        self._packed.invalidate()

    def ok(self, x, parts):
        lin_in, blocks, lin_out = parts
        w = lin_in.weight
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for l in [lin_in, lin_out] + [m for b in blocks for m in b] for p in (l.weight, l.bias))):
            return False      # inference only: no autograd node (ANY trainable layer sends the call to torch's layers, not only a trainable first one)
        return (x.is_cuda and x.dim() == 2 and w.is_cuda and w.dtype == torch.float32 and lin_in.out_features in (128, 256) and lin_in.in_features <= 28
                and lin_out.out_features <= 16 and os.environ.get("D3IL_POLICY_FUSED_RESMLP", "1") == "1")

    @staticmethod
    def _pack_args(parts):
        """(the parameters the packed copy follows, the pack function) for PackedWeights."""
        lin_in, blocks, lin_out = parts
        return [lin_in.weight, lin_in.bias, lin_out.weight, lin_out.bias] + [p for b in blocks for l in b for p in (l.weight, l.bias)], lambda: pack_resmlp_weights(*parts)

    def ensure_packed(self, parts):
        self._packed.ensure(*self._pack_args(parts))

    def __call__(self, x, parts):
        from . import capi
        lin_in, blocks, lin_out = parts
        w = self._packed.current(*self._pack_args(parts))
        x = x.to(torch.float32).contiguous()
        out = torch.empty(x.shape[0], lin_out.out_features, dtype=torch.float32, device=x.device)
        capi.launch("d3il_resmlp_f32", x.device, x=x, **resmlp_args(w), w_out=w["w_out"], b_out=w["b_out"], out=out, rows=x.shape[0], in_dim=lin_in.in_features,
                    hidden=lin_in.out_features, n_blocks=w["n_blocks"], out_dim=lin_out.out_features)
        return out


def capture_graph(fn, device):
    """``fn()`` - a fixed chain of device kernels on static inputs - as a captured HIP graph: two warm-up calls on a side stream (library handles, workspaces and
    lazy initialisation must not happen inside the capture), then the capture.  Returns (graph, static output of fn, the range-guard epoch of the capture)."""
    cur, side = torch.cuda.current_stream(device), torch.cuda.Stream(device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out, _GUARD_EPOCH


def graph_is_stale(epoch, policy) -> bool:
    """A graph holds the kernel instantiation and the counter address of the range-guard setting it was captured under: where split-f16 blocks are involved
    (``policy.f16x3_blocks``) a graph of another _GUARD_EPOCH is dropped and captured again.  Policies without them (BC, DDPM) keep their graph - a new capture
    would also spend their random draws."""
    return epoch != _GUARD_EPOCH and bool(getattr(policy, "f16x3_blocks", False))


class CapturedPolicy:
    """Any policy whose ``predict_batch`` is a fixed chain of device kernels on a fixed batch shape (no host round trip, no data-dependent shapes: BCPolicy,
    the stand-in MLP of agents.py, DDPMPolicy with window_size 1) as ONE captured HIP graph: the first call of a batch shape warms the chain up on a side
    stream and captures it, later calls copy the observation into the graph's static input and replay it on the caller's current stream.  Same kernels, same
    results; the host issues one launch instead of dozens - which is what bounds several sub-batches on several streams.  Random
    draws inside the chain (torch.randn on the device) come from the device generator at every replay.  The returned tensor is the graph's static output:
    consume it before the next call (the rollout loops do)."""

    def __init__(self, inner):
        self.inner = inner
        self._g, self._g_in, self._g_out, self._g_epoch = None, None, None, -1

    def reset(self):
        if hasattr(self.inner, "reset"):
            self.inner.reset()

    def begin_episodes(self, mask):
        if hasattr(self.inner, "begin_episodes"):
            self.inner.begin_episodes(mask)

    def set_rollout_range(self, offset, count):
        if hasattr(self.inner, "set_rollout_range"):
            self.inner.set_rollout_range(offset, count)

    def fork(self):
        """A clone for another sub-batch: the inner policy forked by its own rule, graph and static buffers its own."""
        from .envs.sub_batch import fork_agent
        return CapturedPolicy(fork_agent(self.inner))

    @torch.no_grad()
    def predict_batch(self, obs):
        if not obs.is_cuda:
            return self.inner.predict_batch(obs)
        if self._g is not None and graph_is_stale(self._g_epoch, self.inner):
            self._g = None
        if self._g is None or self._g_in.shape != obs.shape or self._g_in.dtype != obs.dtype:
            self._g_in = obs.clone()
            # a policy with per-episode state on the device (BeTPolicy: history window, step word) hands it over here and gets it back after the capture: the two
            # warm-up calls must not count as steps.  From the snapshot on it runs a fixed-shape chain that updates that state in place.
            snap = self.inner.capture_snapshot(self._g_in) if hasattr(self.inner, "capture_snapshot") else None
            self._g, self._g_out, self._g_epoch = capture_graph(lambda: self.inner.predict_batch(self._g_in), obs.device)
            if snap is not None:
                self.inner.capture_restore(snap)
        if hasattr(self.inner, "ensure_packed"):
            self.inner.ensure_packed()      # packed weight buffers of a fused policy follow the parameters (in place) - e.g. after the EMA swap of a rollout
        self._g_in.copy_(obs)
        self._g.replay()
        return self._g_out


def cosine_beta_schedule(timesteps, s=0.008):     # agents/models/diffusion/utils.py:31-42 (float64 numpy -> float32)
    steps = timesteps + 1
    x = np.linspace(0, steps, steps)
    ac = np.cos(((x / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.tensor(np.clip(1 - (ac[1:] / ac[:-1]), a_min=0, a_max=0.999), dtype=torch.float32)


def ddpm_schedule(betas: torch.Tensor) -> dict:
    """The tables the DDPM samplers derive from the betas (in the betas' dtype, on their device): sqrt(1 / ac), sqrt(1 / ac - 1), the clipped posterior log
    variance, the two posterior-mean coefficients, and ``sched`` [T, 5] = (sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sig) with sig = exp(logvar / 2) and
    sig[0] = 0 - what the fused sampler kernels read per step."""
    alphas = 1.0 - betas
    ac = torch.cumprod(alphas, dim=0)
    ac_prev = torch.cat([torch.ones_like(betas[:1]), ac[:-1]])
    post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
    s = {"betas": betas, "alphas": alphas, "ac": ac, "ac_prev": ac_prev, "sqrt_recip_ac": torch.sqrt(1.0 / ac), "sqrt_recipm1_ac": torch.sqrt(1.0 / ac - 1), "post_var": post_var,
         "post_logvar": torch.log(torch.clamp(post_var, min=1e-20)), "coef1": betas * torch.sqrt(ac_prev) / (1.0 - ac), "coef2": (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac)}
    sig = (0.5 * s["post_logvar"]).exp() * torch.cat((torch.zeros_like(betas[:1]), torch.ones_like(betas[1:])))
    s["sched"] = torch.stack((s["sqrt_recip_ac"], s["sqrt_recipm1_ac"], s["coef1"], s["coef2"], sig), dim=1).contiguous()
    return s


class DDPMPolicy:
    """DiffusionAgent.predict (ddpm_agent.py:213-274) with the Diffusion sampler (gc_diffusion.py:101-216: epsilon prediction, clipped
    x0, posterior mean / variance, n_timesteps ancestral steps, final clamp) on a batch.  ``noise_fn(shape)`` supplies the Gaussian
    noise (default torch.randn on the policy's device); window_size > 1 keeps the observation history per lane.  Non-finite input: an observation row with a
    NaN / Inf (or such a noise draw) gives NaN in both action components of that row on the fused chain as on the torch chain (torch.clamp keeps a NaN; the
    kernel tests the bit patterns, its own clips would return a bound), and no other row changes - the environment then raises D3IL_FLAG_SOLVER_FAIL in that lane."""

    def __init__(self, model: DiffusionMLP, scaler: Scaler, n_timesteps: int, window_size: int = 1, n_envs: int | None = None, noise_fn=None):
        self.model, self.scaler, self.T, self.W = model.eval(), scaler, int(n_timesteps), int(window_size)
        dev = scaler.x_mean.device
        self.device = dev
        sch = ddpm_schedule(cosine_beta_schedule(self.T).to(dev))
        self.sqrt_recip_ac, self.sqrt_recipm1_ac, self.post_logvar, self.coef1, self.coef2, self._sched = (sch[k] for k in ("sqrt_recip_ac", "sqrt_recipm1_ac", "post_logvar", "coef1", "coef2", "sched"))
        self.min_action, self.max_action = scaler.y_bounds[0], scaler.y_bounds[1]
        self._custom_noise = noise_fn is not None
        self.noise_fn = noise_fn or (lambda shape: torch.randn(shape, device=dev))
        self.hist = None
        self.n_envs = n_envs
        self._packed = PackedWeights()

    # ---- the whole chain in one kernel of the rollout library (csrc/policy_f32.h k_ddpm_mlp_f32)
    def fused_ok(self):
        m = self.model
        L = m.layers.layers
        return (self.W <= 1 and isinstance(m, DiffusionMLP) and L[0].weight.is_cuda and L[0].weight.dtype == torch.float32 and L[0].out_features == 256 and L[-1].out_features == 2
                and m.temp_layers[-1].out_features == 8 and 1 <= L[0].in_features - 10 <= 18 and all(isinstance(b, _ResBlock) for b in L[1:-1])
                and os.environ.get("D3IL_POLICY_FUSED_DDPM", "1") == "1")

    def invalidate_packed(self):
        """Force a repack at the next call.  Needed after writes through ``param.data`` (e.g. the reference EMA helper's copy_to / restore), which do not bump the
        version counters ensure_packed() keys on; use_ema() and load_state_dict are seen without it."""
        self._packed.invalidate()
        self.model.layers.invalidate_packed()

    _fw = property(lambda self: self._packed.buf)      # the packed buffers, read-only

    def _pack(self):
        """The denoiser's weights in the tile order of the kernel, the time embeddings of the T steps, the schedule table and the action bounds."""
        self.model.layers.ensure_packed()      # (the torch chain's inner network, if its device path has been used)
        dev = self.model.layers.layers[0].weight.device
        fw = pack_resmlp_weights(*self.model.layers._parts())
        fw["temb"] = self.model.temp_layers(torch.arange(self.T, device=dev)).to(torch.float32).contiguous()
        fw["sched"] = self._sched.to(device=dev, dtype=torch.float32).contiguous()
        fw["bounds"] = torch.cat((self.min_action.reshape(-1), self.max_action.reshape(-1))).to(torch.float32).contiguous()
        return fw

    def ensure_packed(self):
        """The packed buffers of the fused chain (PackedWeights) follow the parameters - e.g. after the EMA swap of a rollout."""
        self._packed.ensure(list(self.model.parameters()), self._pack)

    def _sample_fused(self, state):
        from . import capi
        n, sd = state.shape
        w = self._packed.current(list(self.model.parameters()), self._pack)
        shape = (n, 2)
        noise = torch.stack([self.noise_fn(shape) for _ in range(self.T + 1)]).to(torch.float32).contiguous() if self._custom_noise else torch.randn((self.T + 1, n, 2), device=self.device)
        out = torch.empty(n, 2, dtype=torch.float32, device=self.device)
        capi.launch("d3il_ddpm_mlp_f32", state.device, state=state.contiguous(), noise=noise, temb=w["temb"], **resmlp_args(w), w_out=w["w_out"], b_out=w["b_out"], sched=w["sched"],
                    bounds=w["bounds"], out=out, rows=n, state_dim=sd, n_timesteps=self.T, hidden=256, n_blocks=w["n_blocks"])
        return out

    def fork(self):
        """A clone for another sub-batch (envs/sub_batch.fork_agent): network, scaler and schedule shared, observation history and the packed buffers of the
        fused chain its own (packed again at its first call)."""
        c = copy.copy(self)
        c.hist = copy.deepcopy(self.hist)
        c._packed = PackedWeights()
        return c

    def captured(self):
        """window_size 1: the whole predict chain (input scaling, the T denoising steps with their noise draws - ~60 torch kernels each -, clamp, output scaling)
        as one captured graph (CapturedPolicy)."""
        assert self.W <= 1, "a history window regroups the lanes by history length at every call: not a fixed chain"
        return CapturedPolicy(self)

    def load_reference_state_dict(self, sd):
        """``Diffusion.state_dict()`` of the reference: the denoiser sits under ``model.``."""
        self.model.load_state_dict({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")})

    def use_ema(self, shadow_params):
        swap_in_ema(self.model, shadow_params)

    def reset(self):
        if self.hist is not None:
            self.hist.reset()

    def begin_episodes(self, mask):
        if self.hist is not None:
            self.hist.reset(mask)

    def _sample(self, state):
        shape = (state.shape[0], state.shape[1], self.min_action.shape[0]) if state.dim() == 3 else (state.shape[0], self.min_action.shape[0])
        x = self.noise_fn(shape)
        for i in reversed(range(self.T)):
            t = torch.full((shape[0],), i, device=self.device, dtype=torch.long)
            eps = self.model(x, t, state)
            x0 = (self.sqrt_recip_ac[i] * x - self.sqrt_recipm1_ac[i] * eps).clamp(self.min_action, self.max_action)
            mean = self.coef1[i] * x0 + self.coef2[i] * x
            noise = self.noise_fn(shape)
            x = mean + (0.0 if i == 0 else 1.0) * (0.5 * self.post_logvar[i]).exp() * noise
        return x.clamp(self.min_action, self.max_action)

    @torch.no_grad()
    def predict_batch(self, obs):
        s = self.scaler.scale_input(obs.to(device=self.device, dtype=torch.float32))
        if self.W <= 1:
            if s.is_cuda and s.dim() == 2 and self.fused_ok():
                return self.scaler.inverse_scale_output(self._sample_fused(s))
            return self.scaler.inverse_scale_output(self._sample(s))
        if self.hist is None:
            self.hist = _History(s.shape[0], self.W, s.shape[1], self.device)
        self.hist.append(s)
        out = torch.empty(s.shape[0], self.min_action.shape[0], device=self.device)
        for L, idx in self.hist.groups():
            st = self.hist.buf[:, self.W - L:] if idx is None else self.hist.buf[idx, self.W - L:]
            a = self._sample(st)[:, -1, :]
            if idx is None:
                out = a
            else:
                out[idx] = a
        return self.scaler.inverse_scale_output(out)


class BESOPolicy:
    """BesoAgent.predict (beso_agent.py:316-443) on a batch: observation history (deque maxlen W) and action history (deque maxlen
    W - 1 of the clamped scaled actions), x_T = N(0, sigma_max^2) for the newest action, Euler-ancestral sampling over the linear noise
    schedule (beso_agent.py:122, gc_sampling.py:41-44, 217-256) of the Karras-preconditioned DiffusionGPT (score_wrappers.py:33-99),
    last action of the sequence, clamp, inverse scale."""

    def __init__(self, inner: DiffusionGPT, scaler: Scaler, window_size: int, num_sampling_steps: int, sigma_min: float, sigma_max: float,
                 sigma_data: float = 0.5, noise_fn=None, use_graph: bool = False):
        self.inner, self.scaler, self.W = inner.eval(), scaler, int(window_size)
        # use_graph: capture the sampling loop for full windows ([N, W] sequences, ~1500 small kernels) in a HIP graph and replay it
        # (default noise only: the generator state is part of the capture)
        self.use_graph = bool(use_graph) and noise_fn is None
        self._graph, self._g_epoch = None, -1      # the captured sampling loop and the range-guard epoch (_GUARD_EPOCH) of its capture
        dev = scaler.x_mean.device
        self.device = dev
        self.n_steps, self.sigma_min, self.sigma_max, self.sigma_data = int(num_sampling_steps), float(sigma_min), float(sigma_max), float(sigma_data)
        self.min_action, self.max_action = scaler.y_bounds[0], scaler.y_bounds[1]
        self.noise_fn = noise_fn or (lambda shape: torch.randn(shape, device=dev))
        self.obs_hist = self.act_hist = None
        # the noise schedule as host floats (one transfer here instead of a device synchronisation per sampling step)
        self.sigmas = torch.cat([torch.linspace(self.sigma_max, self.sigma_min, self.n_steps, device=dev), torch.zeros(1, device=dev)]).tolist()

    def load_reference_state_dict(self, sd):
        """``GCDenoiser.state_dict()`` of the reference: the transformer sits under ``inner_model.``."""
        own = self.inner.state_dict()
        self.inner.load_state_dict({k[len("inner_model."):]: v for k, v in sd.items() if k.startswith("inner_model.") and k[len("inner_model."):] in own})

    def use_ema(self, shadow_params):
        swap_in_ema(self.inner, shadow_params)

    f16x3_blocks = True      # the DiffusionGPT blocks run the split-f16 kernels the range guard instruments (CapturedPolicy captures again when the guard changes)

    def weights_out_of_range(self) -> int:
        """Entries of the blocks' f16x3-packed weight matrices that are NaN / Inf or beyond +-65504 (they saturate on the host, policies.split_f16); one
        synchronising read.  Blocks that have not been packed yet are packed first."""
        return blocks_w_oor(self.inner.blocks)

    def range_report(self) -> dict:
        """The active RangeGuard's counters (clipped / nonfinite / launches) plus ``weights_out_of_range``."""
        g = range_guard()
        if g is None:
            raise RuntimeError("range_report: no RangeGuard is enabled (policies.RangeGuard, D3IL_POLICY_RANGE_GUARD=1 or a Sim's policy_range_guard=True)")
        rep = g.read()
        rep["weights_out_of_range"] = self.weights_out_of_range()
        return rep

    def reset(self):
        for h in (self.obs_hist, self.act_hist):
            if h is not None:
                h.reset()

    def begin_episodes(self, mask):
        for h in (self.obs_hist, self.act_hist):
            if h is not None:
                h.reset(mask)

    def _denoise(self, states, actions, sigma: float):
        sd2 = self.sigma_data ** 2
        c_skip, c_out, c_in = sd2 / (sigma ** 2 + sd2), sigma * self.sigma_data / (sigma ** 2 + sd2) ** 0.5, 1 / (sigma ** 2 + sd2) ** 0.5
        s_in = torch.full((actions.shape[0],), sigma, device=self.device)
        return self.inner(states, actions * c_in, s_in) * c_out + actions * c_skip

    def _sample_device(self, states, x):
        """_sample for the device: step-invariant work hoisted (DiffusionGPT.begin_sampling), the Karras combination and the Euler-ancestral update of a step
        merged algebraically - den = c_out net + c_skip x;  x' = x + (x - den) (s_down - s_from) / s_from  =  (1 + k (1 - c_skip)) x - k c_out net  with
        k = (s_down - s_from) / s_from - two element-wise kernels instead of seven (f32 rounding differs from the step-by-step form at the 1e-7 level)."""
        sigmas, sd2 = self.sigmas, self.sigma_data ** 2
        if getattr(self, "_sig_dev", None) is None or self._sig_dev.device != states.device:
            self._sig_dev = torch.tensor(sigmas[:-1], dtype=torch.float32, device=states.device)
        ctx = self.inner.begin_sampling(states, self._sig_dev)
        for i in range(len(sigmas) - 1):
            s_from, s_to = sigmas[i], sigmas[i + 1]
            c_skip, c_out, c_in = sd2 / (s_from ** 2 + sd2), s_from * self.sigma_data / (s_from ** 2 + sd2) ** 0.5, 1 / (s_from ** 2 + sd2) ** 0.5
            net = self.inner.forward_step(ctx, x, i, c_in)
            s_up = min(s_to, (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5)
            s_down = (s_to ** 2 - s_up ** 2) ** 0.5
            k = (s_down - s_from) / s_from
            x = torch.add(x * (1.0 + k * (1.0 - c_skip)), net, alpha=-k * c_out)
            if s_down > 0:
                x = torch.add(x, self.noise_fn(tuple(x.shape)), alpha=s_up)
        return x

    def _sample(self, states, x):
        if states.is_cuda and os.environ.get("D3IL_POLICY_BESO_FUSED_GLUE", "1") == "1" and not (torch.is_grad_enabled() and any(p.requires_grad for p in self.inner.parameters())):
            return self._sample_device(states, x)
        sigmas = self.sigmas
        for i in range(len(sigmas) - 1):
            s_from, s_to = sigmas[i], sigmas[i + 1]
            den = self._denoise(states, x, s_from)
            s_up = min(s_to, (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5)
            s_down = (s_to ** 2 - s_up ** 2) ** 0.5
            x = x + (x - den) / s_from * (s_down - s_from)
            if s_down > 0:
                x = x + self.noise_fn(tuple(x.shape)) * s_up
        return x

    def _sample_full(self, states, x):
        """``_sample`` for full windows; with ``use_graph`` one HIP-graph replay instead of the eager kernel sequence."""
        if not (self.use_graph and states.is_cuda and states.shape[1] == self.W):
            return self._sample(states, x)
        if self._graph is None or self._g_st.shape != states.shape or graph_is_stale(self._g_epoch, self):
            self._g_st, self._g_x = states.clone(), x.clone()
            self._graph, self._g_out, self._g_epoch = capture_graph(lambda: self._sample(self._g_st, self._g_x), states.device)
        self._g_st.copy_(states); self._g_x.copy_(x)
        self._graph.replay()
        return self._g_out

    def _padded_inputs(self, noise):
        """The padded observation window (_History.padded) and, aligned with it, the action sequence: the previous actions of lane i at positions 0 .. len_i - 2,
        the noise of its newest action at position len_i - 1."""
        W = self.W
        st, L = self.obs_hist.padded()
        j = torch.arange(W, device=self.device)
        newest = (j == (L - 1).unsqueeze(1)).unsqueeze(2)
        x = newest * noise
        if self.act_hist is not None:
            srca = ((W - L).unsqueeze(1) + j).clamp(0, W - 2)
            xa = torch.gather(self.act_hist.buf, 1, srca.unsqueeze(2).expand(-1, -1, self.act_hist.buf.shape[2]))
            x = x + xa * (j < (L - 1).unsqueeze(1)).unsqueeze(2)
        return st, x

    @torch.no_grad()
    def predict_batch(self, obs):
        s = self.scaler.scale_input(obs.to(device=self.device, dtype=torch.float32))
        n, act_dim = s.shape[0], self.min_action.shape[0]
        if s.is_cuda and getattr(self, "_sig_dev", None) is None:
            self._sig_dev = torch.tensor(self.sigmas[:-1], dtype=torch.float32, device=s.device)      # (made here, outside a captured sampling loop)
        if s.is_cuda and not _ENV_GUARD_TRIED and policy_gemm_mode() == "f16x3":
            _env_range_guard(s.device)
        if s.is_cuda:                          # packed weight copies of the fused blocks: refreshed here, OUTSIDE a captured sampling loop
            ensure_blocks_packed(self.inner.blocks)
        if self.obs_hist is None:
            self.obs_hist = _History(n, self.W, s.shape[1], self.device)
            self.act_hist = _History(n, self.W - 1, act_dim, self.device) if self.W > 1 else None
        self.obs_hist.append(s)
        noise = self.noise_fn((n, 1, act_dim)) * self.sigma_max
        L = self.obs_hist.lockstep
        if L >= 0:                             # all lanes have the same history length: the reference's shapes
            st = self.obs_hist.buf[:, self.W - L:]
            x = noise
            if L > 1:                          # previous actions: the action deque holds min(L - 1, W - 1) entries
                x = torch.cat([self.act_hist.buf[:, (self.W - 1) - (L - 1):], x], dim=1)
            x0_all = self._sample_full(st, x)[:, -1, :].clamp(self.min_action, self.max_action)
        else:                                  # lanes restarted at different times: one padded batch, no host synchronisation
            st, x = self._padded_inputs(noise)
            out = self._sample_full(st, x)
            x0_all = out.gather(1, (self.obs_hist.len - 1).view(n, 1, 1).expand(-1, 1, act_dim)).squeeze(1).clamp(self.min_action, self.max_action)
        if self.act_hist is not None:
            self.act_hist.append(x0_all)
            self.act_hist.len = (self.obs_hist.len - 1).clamp_min(0).clamp_max(self.W - 1)
            self.act_hist.lockstep = -1 if self.obs_hist.lockstep < 0 else min(max(self.obs_hist.lockstep - 1, 0), self.W - 1)
        return self.scaler.inverse_scale_output(x0_all)


# ------------------------------------------------------------------------------------------------ the Philox stream of the native policies, on the host
def philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 on numpy arrays / ints (broadcast): the four output words as uint32 arrays - the host form of csrc/policy_common.h philox4x32_10."""
    m32 = np.uint64(0xFFFFFFFF)
    u = lambda v: np.asarray(v, dtype=np.uint64) & m32
    k0, k1, c0, c1, c2, c3 = np.broadcast_arrays(u(k0), u(k1), u(c0), u(c1), u(c2), u(c3))
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + W0) & m32, (k1 + W1) & m32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def philox_words(seed: int, env_offset: int, n: int, t: int, tag):
    """THE stream of every native policy: uint32 [n, ..., 4] = Philox4x32-10(key = (lo32, hi32 of seed), counter = (lo32, hi32 of env_offset + row, t, tag)) for rows
    0 .. n-1.  ``tag`` - the policy's *_TAG or-ed with its layout bits - is a uint64 scalar or an array [1, ...] that broadcasts against the row axis."""
    tag = np.asarray(tag, dtype=np.uint64)
    ge = (np.uint64(env_offset) + np.arange(n, dtype=np.uint64)).reshape((n,) + (1,) * (tag.ndim - 1))
    return np.stack(philox4x32_10(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, ge & np.uint64(0xFFFFFFFF), ge >> np.uint64(32), t & 0xFFFFFFFF, tag), axis=-1)


def uniform24(r):
    """The upper 24 bits of Philox words as float32 uniforms in [0, 1 - 2^-24] (csrc/policy_common.h policy_uniform24)."""
    return ((r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def box_muller_f64(r):
    """Standard normals from Philox words [..., 4], float64 [..., 4]: exact on the words and f64 from there on (csrc/policy_common.h policy_box_muller in f32):
    u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, (n0, n1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2); (n2, n3) likewise from r2, r3."""
    out = np.zeros(r.shape)
    for p in range(2):
        u1 = ((r[..., 2 * p] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (r[..., 2 * p + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        rad = np.sqrt(-2.0 * np.log(u1))
        out[..., 2 * p], out[..., 2 * p + 1] = rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)
    return out


def _tag_axes(*sizes):
    """uint64 index arrays [1, s0, 1, ..], [1, 1, s1, ..], .. for the layout bits of a tag: one axis per size behind the row axis."""
    return [np.arange(s, dtype=np.uint64).reshape((1,) * (i + 1) + (s,) + (1,) * (len(sizes) - 1 - i)) for i, s in enumerate(sizes)]


def _first_parameter(module):
    """``next(module.parameters())`` without the generator chain of nn.Module (this runs in every eager policy step)."""
    for p in module._parameters.values():
        if p is not None:
            return p
    for child in module._modules.values():
        p = _first_parameter(child)
        if p is not None:
            return p
    return None


class NativePolicy:
    """What the Sims, SubBatchSet and CapturedPolicy call on a policy that draws from the Philox stream above, and the steps every such policy takes, written
    once.  A subclass has ``model`` (the network), ``scaler``, ``device`` and ``obs_dim``, calls ``_init_output(scaler)`` and ``_init_stream(seed)`` in its
    constructor and states
      SWITCH   the D3IL_POLICY_* variable that turns its kernel off ("0": the torch path, which the tests compare the kernel against);
      STATE    the names of its per-lane device tensors (None until ``_state(n)`` has sized them);  ``hist``, a _History or None, is per-lane state too;
      LAST     the names of the ``last_*`` records a fork starts without;
      TAKES    what reads the observation row, for the width check ("the decoder takes %d next to its latent");
      BOUNDS   the attribute names of its clamp bounds (BeT, BC-GPT and DDPM-GPT say ``min_action`` / ``max_action``);
      _state(n)                 make the per-lane state fit n lanes (default: there is none);
      _kernel_shape()           is the network one its kernel is built for?  Only then is it packed and launched;
      _pack()                   the packer for PackedWeights (_pack_params(): the parameters the tables follow, default all of the model's);
      _step_kernel(s)           one step on the scaled observations s [N, obs_dim] through its row of capi.SIGNATURES (capi.launch, by name);
      _step_torch(s)            the same arithmetic as torch ops (``_draw`` for the random numbers, ``_action_tail`` for the end);
      _fallback_text()          what the once-per-policy warning says when the kernel is on and does not apply.
    ``predict_batch`` is then the template below; a policy that drives a trunk between its history and its tail (BeT, DDPM-GPT) writes its own.
    The step word ``_t`` lives on the device (the kernels read it as u32); a captured graph advances it at every replay."""

    SWITCH, STATE, LAST, TAKES, BOUNDS = None, (), (), "the network takes %d", ("lo", "hi")
    hist = None

    def _init_stream(self, seed):
        self.seed, self.env_offset = int(seed), 0
        self._t = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._packed = PackedWeights()

    def _init_output(self, scaler, lo=None, hi=None):
        """The constants of the action tail, f32 on the device: the clamp bounds in scaled space (default: the scaler's ``y_bounds``) under the names BOUNDS, and
        ``out_scale`` / ``out_shift`` of the inverse scaling."""
        f = lambda a: torch.as_tensor(a).detach().to(device=self.device, dtype=torch.float32).contiguous()
        setattr(self, self.BOUNDS[0], f(scaler.y_bounds[0] if lo is None else lo))
        setattr(self, self.BOUNDS[1], f(scaler.y_bounds[1] if hi is None else hi))
        self.out_scale, self.out_shift = f(scaler.y_std + 1e-12), f(scaler.y_mean)

    def _state(self, n):
        pass

    def reset(self):
        pass

    def _kernel_shape(self) -> bool:
        return True

    def _switch_on(self) -> bool:
        return os.environ.get(self.SWITCH, "1") == "1"

    def _pack_params(self):
        return list(self.model.parameters())

    def fused_ok(self, s) -> bool:
        w = _first_parameter(self.model)
        return s.is_cuda and w.is_cuda and w.dtype == torch.float32 and self._kernel_shape() and self._switch_on()

    def _draw_args(self) -> dict:
        """The keywords every drawing kernel takes: tail constants, Philox key, rollout offset, step word."""
        return dict(lo=getattr(self, self.BOUNDS[0]), hi=getattr(self, self.BOUNDS[1]), scale=self.out_scale, shift=self.out_shift, seed=self.seed, env_offset=self.env_offset, t_device=self._t)

    @torch.no_grad()
    def predict_batch(self, obs):
        s = self.scaler.scale_input(obs.to(device=self.device, dtype=torch.float32)).contiguous()
        assert s.dim() == 2 and s.shape[1] == self.obs_dim, "%s: observation width %d, %s" % (type(self).__name__, s.shape[-1], self.TAKES % self.obs_dim)
        self._state(s.shape[0])
        if self.fused_ok(s):
            y = self._step_kernel(s)
        else:
            self._warn_fallback(s, self._fallback_text)
            y = self._step_torch(s)
        self._t.add_(1)
        return y

    def set_rollout_range(self, offset, count):
        """Rows 0 .. count-1 of this policy's batch are rollouts offset .. offset+count-1: the Philox counter of row i is env_offset + i."""
        self.env_offset = int(offset)
        self._state(int(count))

    def fork(self):
        """A clone for another sub-batch: network, scaler and tables shared; per-lane state, step word and packed buffers its own."""
        c = copy.copy(self)
        c._t, c._packed = self._t.clone(), PackedWeights()
        for k in self.STATE:
            setattr(c, k, None if getattr(self, k) is None else getattr(self, k).clone())
        c.hist = None if self.hist is None else self.hist.copy()
        for k in self.LAST:
            setattr(c, k, None)
        return c

    def captured(self):
        """This policy as one captured HIP graph per batch shape (the kernel path is a fixed chain that ends with the add on the step word)."""
        return CapturedPolicy(self)

    def use_ema(self, shadow_params):
        swap_in_ema(self.model, shadow_params)

    def invalidate_packed(self):
        """After ``param.data`` writes (invisible to the version counters): the next call / ensure_packed() repacks."""
        self._packed.invalidate()

    def ensure_packed(self):
        if next(self.model.parameters()).is_cuda and self._kernel_shape():
            self._packed.ensure(self._pack_params(), self._pack)

    # ---- CapturedPolicy's hooks
    def capture_snapshot(self, obs):
        """Before the warm-up calls of a capture: the per-lane state and the step word, which capture_restore puts back - warm-up and capture do not count as steps."""
        self._state(int(obs.shape[0]))
        return [getattr(self, k).clone() for k in ("_t",) + self.STATE], None if self.hist is None else self.hist.snapshot()

    def capture_restore(self, snap):
        tensors, hist = snap
        for k, src in zip(("_t",) + self.STATE, tensors):
            getattr(self, k).copy_(src)
        if hist is not None:
            self.hist.restore(hist)

    # ---- the torch paths
    def _host_step_word(self) -> int:
        """The step word for a draw on the host (a device synchronisation) - which a graph capture cannot record."""
        if torch.cuda.is_initialized() and _capturing():
            raise RuntimeError("%s: the torch path draws its Philox numbers on the host and cannot be captured; the kernel draws on the device" % type(self).__name__)
        return int(self._t.item()) & 0xFFFFFFFF

    def _draw(self, given_fn, n, shape, host_draw, need_host: bool, dev):
        """A bank of random numbers, f32 ``shape`` on ``dev``, as the torch path takes it / as the kernel is handed it: ``given_fn(n)`` where the policy was given
        one, or (``need_host``) ``host_draw(step word)`` - the host form of the kernel's own draw -, or None: the kernel draws."""
        if given_fn is not None:
            return torch.as_tensor(given_fn(n), dtype=torch.float32).to(dev).reshape(shape).contiguous()
        if not need_host:
            return None
        return torch.as_tensor(host_draw(self._host_step_word()), dtype=torch.float32).to(dev)

    def _action_tail(self, x, bad, f64: bool, lo=None, hi=None, dt=None):
        """The end of every torch path: clamp ``x`` [N, .., A] to [lo, hi] in its dtype (None: the caller has clamped, or there is no clamp), scale and shift, NaN
        for the rows marked in ``bad`` [N].  ``f64``: the product and the sum in f64, rounded once to ``dt`` (default: the dtype of x) - what the kernels of CVAE,
        BeT-MLP, BC-GPT and IBC do; otherwise both in ``dt``, rounded twice - BeT, DDPM-GPT, ACT, DDPM-ACT."""
        dt = x.dtype if dt is None else dt
        if lo is not None:
            x = torch.minimum(torch.maximum(x, lo.to(x.device, x.dtype)), hi.to(x.device, x.dtype))
        wide = torch.float64 if f64 else dt
        y = (x.to(wide) * self.out_scale.to(x.device, wide) + self.out_shift.to(x.device, wide)).to(dt)
        return torch.where(bad.bool().reshape((-1,) + (1,) * (y.dim() - 1)), torch.full_like(y, float("nan")), y)

    def _warn_fallback(self, s, text):
        """Once per policy (forks copy the flag): the kernel is switched on, the input is on the device, and this network is not one it is built for."""
        if s.is_cuda and self._switch_on() and not getattr(self, "_warned", False):
            self._warned = True
            warnings.warn("%s: %s" % (type(self).__name__, text()))


class _ChunkLanes:
    """The per-lane bookkeeping of the policies that emit action chunks (ACT, DDPM-ACT), in front of NativePolicy: ``counter`` i32 [N] and ``chunk`` f32
    [N, chunk length, A] (clamped, inverse-scaled) on the device.  A lane whose counter equals the chunk length (or lies outside 0 .. length) is due."""

    def _chunk_state(self, n, length):
        self.counter = torch.full((n,), length, dtype=torch.int32, device=self.device)
        self.chunk = torch.zeros(n, length, self.A, dtype=torch.float32, device=self.device)

    def _due(self):
        return (self.counter >= self.chunk.shape[1]) | (self.counter < 0)

    def _emit(self):
        """chunk[counter] of every lane; the counters count on."""
        y = self.chunk[torch.arange(self.chunk.shape[0], device=self.chunk.device), self.counter.long()]
        self.counter.add_(1)
        return y

    def reset(self):
        """The agent's reset for every lane: empty windows, the next call computes a chunk everywhere."""
        if self.counter is not None:
            self.counter.fill_(self.chunk.shape[1])
            if self.hist is not None:
                self.hist.reset()

    def begin_episodes(self, mask):
        """Lanes that start a new trajectory: window length 0, due at their next step (in place on the device, also under a captured graph)."""
        self._state(int(mask.shape[0]))
        m = mask.to(device=self.device, dtype=torch.bool).reshape(-1)
        self.counter.masked_fill_(m, self.chunk.shape[1])
        if self.hist is not None:
            self.hist.reset_(m)

    def predict_batch(self, obs):
        y = super().predict_batch(obs)
        if self.record:
            self.last_chunk = self.chunk.clone()      # a copy of the chunk table after every call
        return y


# ------------------------------------------------------------------------------------------------ Behaviour Transformer
BET_TAG = 0x42655448          # fourth Philox counter word of the sampling head (csrc/policy_bet.h BET_TAG; the random-policy harness uses 0)


def bet_uniforms(seed: int, env_offset: int, n: int, t: int):
    """The head kernel's uniforms of rows 0 .. n-1 at step word t, on the host: 24 bits of Philox4x32-10(key = seed, counter = (env_offset + row, t, BET_TAG)),
    float32 in [0, 1 - 2^-24]."""
    return uniform24(philox_words(seed, env_offset, n, t, BET_TAG)[:, 0])


class MinGPTTrunk(nn.Module):
    """The GPT of the reference's BeT (agents/models/bet/libraries/mingpt/model.py:128-250; continuous input, eval mode) with the reference's parameter names -
    ``tok_emb``, ``pos_emb``, ``blocks.N.(ln1 | attn.key / query / value / proj | ln2 | mlp.0 / mlp.2)``, ``ln_f``, ``head`` (no bias, V (1 + A) outputs) - so
    ``load_state_dict`` of a reference state dict works.  The blocks are ``_Block``, walked by ``run_blocks``: 120-wide trunks on the device take the matrix-core kernels
    of the DiffusionGPT, 72-wide 4-head trunks the one-launch trunk kernel, every other shape runs the same blocks through torch, batched.  ``hidden`` stops BEFORE ``ln_f``: the final LayerNorm and the head belong to the sampling tail."""

    def __init__(self, input_dim, n_embd, n_layer, n_head, block_size, vocab_size=64, action_dim=0):
        super().__init__()
        self.tok_emb = nn.Linear(input_dim, n_embd)
        self.pos_emb = nn.Parameter(torch.zeros(1, block_size, n_embd))
        self.blocks = nn.Sequential(*[_Block(n_embd, n_head, block_size) for _ in range(n_layer)])
        self.ln_f = nn.LayerNorm(n_embd)
        self.head = nn.Linear(n_embd, vocab_size * (1 + action_dim), bias=False)
        self.block_size, self.n_embd, self.vocab_size, self.action_dim = block_size, n_embd, vocab_size, action_dim

    def hidden(self, x, keep=None):
        """x [N, T, input_dim] -> the last block's output [N, T, C], or [N, len(keep), C] for the token positions ``keep`` (attention sees every token; the last
        block's projection and MLP run on the kept rows only)."""
        t = x.shape[1]
        assert t <= self.block_size, "Cannot forward, model block size is exhausted."
        h = (self.tok_emb(x) + self.pos_emb[:, :t, :]).contiguous()
        return run_blocks(self.blocks, h, keep=keep)

    def forward(self, x):
        """The reference's GPT.forward without targets: [N, T, V (1 + A)]."""
        return self.head(self.ln_f(self.hidden(x)))


class BeTPolicy(NativePolicy):
    """BeT_Agent.predict (agents/bet_agent.py:328-384) on a batch: scaled observation window (deque maxlen W; the window GROWS at episode start - sequence length
    1, 2, .. W with pos_emb[:L]), the minGPT trunk, and at every lane's last token the sampling tail - ln_f, the bias-free head of V (1 + A) outputs, softmax over the
    first V, ONE categorical draw, the offsets of the drawn bin in the layout "(V A)" (latent_generators/mingpt.py:155-186), bin_centers[bin] + offset (k_means.py:111-138),
    clamp to the data bounds IN SCALED SPACE, inverse scaling.

    The draw is the inverse CDF of the un-normalised softmax, bin = min(#{v : c_v <= u S}, V - 1) with c the inclusive prefix sums of p = exp(logit - max) and S = c_{V-1},
    on ONE uniform u per lane and step: 24 bits of Philox4x32-10 keyed by ``seed`` with counter (env_offset + lane, step word, BET_TAG) - independent of batch order,
    sub-batches and rank count, unlike torch.multinomial's device generator - or ``uniform_fn(n) -> [n]`` when given (golden replay, tests).  The step word lives on
    the device and is advanced by a device-side add after every call, so a captured graph (CapturedPolicy) draws fresh numbers at every replay.

    Deliberately dropped: the reference draws bins for the L - 1 EARLIER positions of the window too (generate_latents samples every row of [batch seq]) and throws
    them away (bet_agent.py:364); that consumes its generator and nothing else.

    On a HIP device the tail is one kernel (csrc/policy_bet.h through d3il_bet_head_f32; V = 64, C <= 128, A <= 8); on the CPU, for other shapes and with
    D3IL_POLICY_BET_HEAD=0 the same arithmetic as torch ops (``_tail_torch``).  Lanes with different history lengths (after ``begin_episodes(mask)``) run in one
    right-padded batch and each lane reads the trunk at its own last valid position - causal attention never looks at the padding behind it."""

    def __init__(self, trunk: MinGPTTrunk, bin_centers, scaler: Scaler, min_action, max_action, window_size: int, seed: int = 0, uniform_fn=None):
        self.trunk, self.scaler, self.W = trunk.eval(), scaler, int(window_size)
        dev = scaler.x_mean.device
        self.device = dev
        f = lambda a: torch.as_tensor(a, device=dev).detach().to(torch.float32).contiguous()
        self.centers = f(bin_centers)
        self.V, self.A = int(self.centers.shape[0]), int(self.centers.shape[1])
        assert trunk.head.weight.shape[0] == self.V * (1 + self.A), "the head has V (1 + A) outputs"
        self._init_output(scaler, min_action, max_action)
        self._init_stream(seed)
        self.uniform_fn = uniform_fn
        self.hist = None
        self._static = False          # fixed-shape chain with device-only state (set by capture_snapshot)
        self.record = False           # also keep the head's probabilities (last_probs) / the torch tail's logits (last_logits)
        self.last_bins = self.last_u = self.last_probs = self.last_logits = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, uniform_fn=None, device=None):
        """From a live reference ``BeT_Agent`` (duck-typed): ``agent.model.model.model.state_dict()`` (the GPT), ``agent.action_ae.bin_centers``, ``agent.scaler``
        (x_mean / x_std / y_mean / y_std), ``agent.min_action`` / ``max_action``, ``agent.window_size``."""
        mingpt = agent.model.model
        sd = mingpt.model.state_dict()
        dev = torch.device(device) if device is not None else sd["tok_emb.weight"].device
        n_embd, input_dim = sd["tok_emb.weight"].shape
        n_layer = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        centers = torch.as_tensor(agent.action_ae.bin_centers)
        V, A = centers.shape
        n_head = int(getattr(mingpt, "n_head", 0) or mingpt.model.blocks[0].attn.n_head)
        trunk = MinGPTTrunk(input_dim, n_embd, n_layer, n_head, sd["pos_emb"].shape[1], V, A)
        trunk.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        trunk = trunk.to(dev).requires_grad_(False)
        return cls(trunk, centers, Scaler.from_reference(agent.scaler, dev, bounds_optional=True), agent.min_action, agent.max_action, int(agent.window_size), seed=seed, uniform_fn=uniform_fn)

    @staticmethod
    def matches(agent) -> bool:
        """Does ``agent`` look like the reference's BeT_Agent (what from_reference reads)?"""
        try:
            return (hasattr(agent.model.model.model, "state_dict") and hasattr(agent.action_ae, "bin_centers") and hasattr(agent, "scaler")
                    and hasattr(agent, "min_action") and hasattr(agent, "max_action") and hasattr(agent, "window_size"))
        except AttributeError:
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy)
    SWITCH, LAST, BOUNDS = "D3IL_POLICY_BET_HEAD", ("last_bins", "last_u", "last_probs", "last_logits"), ("min_action", "max_action")
    model = property(lambda self: self.trunk)

    @property
    def f16x3_blocks(self) -> bool:
        """The trunk runs the split-f16 kernels the range guard instruments (CapturedPolicy captures again when the guard changes)."""
        return blocks_f16x3(self.trunk.blocks)

    def _state(self, n):
        """The observation window for n lanes; a new size starts empty."""
        if self.hist is None or self.hist.buf.shape[0] != n:
            self.hist = _History(n, self.W, self.trunk.tok_emb.in_features, self.device)

    def reset(self):
        if self.hist is not None:
            self.hist.reset()

    def begin_episodes(self, mask):
        if self.hist is not None:
            self.hist.reset_(mask)

    def fork(self):
        """A clone for another sub-batch: trunk, head, centres and scaler shared; step word its own, an empty history, not in capture mode."""
        c = super().fork()
        c.hist, c._static = None, False
        return c

    def invalidate_packed(self):
        invalidate_blocks_packed(self.trunk.blocks)

    def ensure_packed(self):
        """The packed weights are the blocks' own."""
        ensure_blocks_packed(self.trunk.blocks)

    def load_reference_state_dict(self, sd):
        """``GPT.state_dict()`` of the reference (bet_agent.py: agent.model.model.model)."""
        self.trunk.load_state_dict(sd)

    # ---- CapturedPolicy's hooks
    def capture_snapshot(self, obs):
        """Also switches to the fixed-shape chain (right-padded windows, lengths on the device, in-place history)."""
        self._static = True
        return super().capture_snapshot(obs)

    # ---- the sampling tail
    def head_kernel_ok(self, h) -> bool:
        C = h.shape[-1]
        return (h.is_cuda and h.dtype == torch.float32 and self.V == 64 and C <= 128 and C % 4 == 0 and 1 <= self.A <= 8 and self.trunk.head.weight.dtype == torch.float32
                and self._switch_on())

    def _uniforms(self, n, dev, need_host: bool = True):
        return self._draw(self.uniform_fn, n, (n,), lambda t: bet_uniforms(self.seed, self.env_offset, n, t), need_host, dev)

    def _tail_torch(self, h):
        """Steps 1 - 7 of csrc/policy_bet.h as torch ops, in the kernel's order of operations where the order is defined (S is the last prefix sum)."""
        n, V, A = h.shape[0], self.V, self.A
        w = self.trunk.head.weight
        x = self.trunk.ln_f(h)
        logits = F.linear(x, w[:V])
        p = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        c = torch.cumsum(p, dim=1)
        S = c[:, -1:]
        u = self._uniforms(n, h.device)
        bins = (c <= u.unsqueeze(1) * S).sum(dim=1).clamp_max(V - 1)
        rows = V + bins.unsqueeze(1) * A + torch.arange(A, device=h.device)
        off = (w[rows] * x.unsqueeze(1)).sum(dim=2)
        bad = ~torch.isfinite(h).all(dim=1)
        y = self._action_tail(torch.clamp(self.centers[bins] + off, self.min_action, self.max_action), bad, f64=False)
        self.last_bins, self.last_u = torch.where(bad, torch.full_like(bins, -1), bins).to(torch.int32), u
        if self.record:
            self.last_logits, self.last_probs = logits, p / S
        return y

    def _tail_kernel(self, h):
        from . import capi
        n, C = h.shape
        h = h.contiguous()
        dev = h.device
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        bins = torch.empty(n, dtype=torch.int32, device=dev)
        u_out = torch.empty(n, dtype=torch.float32, device=dev)
        probs = torch.empty(n, self.V, dtype=torch.float32, device=dev) if self.record else None
        ln, w = self.trunk.ln_f, self.trunk.head.weight
        assert w.is_contiguous()
        capi.launch("d3il_bet_head_f32", dev, h=h, ln_weight=ln.weight, ln_bias=ln.bias, ln_eps=float(ln.eps), w_head=w, centers=self.centers, **self._draw_args(),
                    u_in=self._uniforms(n, dev, False), actions=y, bins=bins, u_out=u_out, probs=probs, rows=n, C=C, V=self.V, A=self.A)
        self.last_bins, self.last_u, self.last_probs, self.last_logits = bins, u_out, probs, None
        return y

    def tail(self, h):
        """h [N, C] (the trunk's output at every lane's last token, before ln_f) -> actions [N, A]; advances the step word."""
        y = self._tail_kernel(h) if self.head_kernel_ok(h) else self._tail_torch(h)
        self._t.add_(1)
        return y

    def _last_hidden(self):
        W, hist = self.W, self.hist
        L = -1 if self._static else hist.lockstep      # (as BESOPolicy: no host look at the lengths once lanes have restarted)
        if L >= 0:                              # all lanes have the same history length: the reference's shapes, only the last token leaves the last block
            if getattr(self, "_keep", None) is None or self._keep.device != hist.buf.device:
                self._keep = torch.arange(W, device=hist.buf.device)
            return self.trunk.hidden(hist.buf[:, W - L:], keep=self._keep[L - 1:L])[:, 0]
        st, ln = hist.padded()
        out = self.trunk.hidden(st)
        return out.gather(1, (ln - 1).view(-1, 1, 1).expand(-1, 1, out.shape[2])).squeeze(1)

    @torch.no_grad()
    def predict_batch(self, obs):
        s = self.scaler.scale_input(obs.to(device=self.device, dtype=torch.float32))
        if s.is_cuda and not _ENV_GUARD_TRIED and self.f16x3_blocks:
            _env_range_guard(s.device)
        if s.is_cuda and not _capturing():
            self.ensure_packed()
        self._state(s.shape[0])
        self.hist.append_(s)
        return self.tail(self._last_hidden().contiguous())

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, n_embd: int = 120, n_layer: int = 6, n_head: int = 6, window_size: int = 5,
               action_scale: float = 0.002, uniform_fn=None, policy_seed: int = 0):
        """A BeT policy of the reference's Stacking / Sorting-4 shape (n_layer 6, n_head 6, n_embd 120, window 5, 64 bins) with fixed random weights - there are no
        checkpoints offline (as agents.RandomResidualMLPPolicy): torch's default layer initialisation, logit weights scaled to a standard deviation of ~2 (a
        distribution that is neither uniform nor one-hot), unit observation scaling, actions of ``action_scale`` per unit of the scaled space, bounds +-1.5."""
        g = torch.Generator().manual_seed(seed)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            trunk = MinGPTTrunk(obs_dim, n_embd, n_layer, n_head, window_size, 64, action_dim)
        with torch.no_grad():
            trunk.pos_emb.copy_(torch.randn(trunk.pos_emb.shape, generator=g) * 0.1)
            trunk.head.weight[:64] = torch.randn(64, n_embd, generator=g) * (2.0 / n_embd ** 0.5)
            trunk.head.weight[64:] = torch.randn(64 * action_dim, n_embd, generator=g) * (0.4 / n_embd ** 0.5)
        sc = Scaler.unit(obs_dim, action_dim, action_scale, 1.5, device)
        return cls(trunk.requires_grad_(False).to(device), torch.randn(64, action_dim, generator=g) * 0.9, sc, sc.y_bounds[0], sc.y_bounds[1], window_size, seed=policy_seed, uniform_fn=uniform_fn)


# ------------------------------------------------------------------------------------------------ DDPM with the transformer denoiser
DDPM_GPT_TAG = 0x44470000     # fourth Philox counter word of the step kernel, or-ed with k << 8 | j << 1 | q (csrc/policy_ddpm_gpt.h; never 0, never BET_TAG)


def ddpm_gpt_words(seed: int, env_offset: int, n: int, t: int, k: int, W: int):
    """The Philox words behind ``ddpm_gpt_normals``: uint32 [n, W, 2 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t,
    DDPM_GPT_TAG | k << 8 | j << 1 | q))."""
    assert 1 <= k <= 255 and 1 <= W <= 16, "the counter layout holds k <= 255 and j <= 15; chain index 0 is never drawn"
    j, q = _tag_axes(W, 2)
    return philox_words(seed, env_offset, n, t, np.uint64(DDPM_GPT_TAG | (k << 8)) | (j << np.uint64(1)) | q)


def ddpm_gpt_normals(seed: int, env_offset: int, n: int, t: int, k: int, W: int, A: int):
    """The step kernel's normals of environments 0 .. n-1 at step word t and chain index k, on the host: float64 [n, W, A].  Exact on the 32-bit words
    (``ddpm_gpt_words``: two calls q per (row, j)) and f64 from there on (``box_muller_f64``); component a = 4 q + m."""
    assert 1 <= A <= 8
    return box_muller_f64(ddpm_gpt_words(seed, env_offset, n, t, k, W)).reshape(n, W, 8)[:, :, :A]


class DiffusionGPTDenoiser(nn.Module):
    """DiffusionTransformerNetwork (agents/models/diffusion/diffusion_models.py:409-667), not goal conditioned, with the reference's parameter names - ``tok_emb``,
    ``pos_emb``, ``blocks.N...``, ``ln_f``, ``time_emb.1 / .3``, ``action_emb``, ``action_pred`` - so the entries of ``Diffusion.state_dict()`` under ``model.``
    load with ``load_state_dict``.  It is DiffusionGPT with the time-step MLP (SinusoidalPosEmb(C) -> Linear(C, 2 C) -> Mish -> Linear(2 C, C)) in place of
    ``sigma_emb``: tokens [time, s_1, a_1, ..., s_t, a_t], the same ``_Block`` (120-wide nets take the matrix-core kernels), the action positions are decoded."""

    def __init__(self, state_dim, action_dim, embed_dim, n_layers, n_heads, obs_seq_len, linear_output=True):
        super().__init__()
        block_size = 2 * obs_seq_len + 1
        self.tok_emb = nn.Linear(state_dim, embed_dim)
        self.pos_emb = nn.Parameter(torch.zeros(1, obs_seq_len + 1, embed_dim))
        self.blocks = nn.Sequential(*[_Block(embed_dim, n_heads, block_size) for _ in range(n_layers)])
        self.ln_f = nn.LayerNorm(embed_dim)
        self.time_emb = nn.Sequential(_SinusoidalPosEmb(embed_dim), nn.Linear(embed_dim, embed_dim * 2), nn.Mish(), nn.Linear(embed_dim * 2, embed_dim))
        self.action_emb = nn.Linear(action_dim, embed_dim)
        self.action_pred = nn.Linear(embed_dim, action_dim) if linear_output else nn.Sequential(nn.Linear(embed_dim, 100), nn.GELU(), nn.Linear(100, action_dim))
        self.goal_conditioned = False
        self.state_dim, self.action_dim, self.obs_seq_len, self.embed_dim, self.n_heads, self.linear_output = state_dim, action_dim, obs_seq_len, embed_dim, n_heads, bool(linear_output)

    def hidden(self, xbuf, keep):
        """The block chain on a token buffer [b, 2 t + 1, C]: the last block's output at the positions ``keep`` (before ln_f)."""
        return run_blocks(self.blocks, xbuf, keep=keep)

    def forward(self, actions, time, states, goals=None):
        """The reference's forward without goals: eps [b, t, A] for actions [b, t, A], time [b] (integers) and states [b, t, state_dim]."""
        b, t, _ = states.size()
        emb_t = self.time_emb(time.reshape(b)).unsqueeze(1)
        pos = self.pos_emb[:, :t, :]
        state_x, action_x = self.tok_emb(states) + pos, self.action_emb(actions) + pos
        sa = torch.stack([state_x, action_x], dim=1).permute(0, 2, 1, 3).reshape(b, 2 * t, self.embed_dim)
        x = torch.cat([emb_t, sa], dim=1).contiguous()
        keep = torch.arange(2, 2 * t + 1, 2, device=x.device)
        return self.action_pred(_layer_norm(self.ln_f, self.hidden(x, keep).contiguous()))


class DDPMGPTPolicy(NativePolicy):
    """DiffusionAgent.predict with window_size > 1 (agents/ddpm_agent.py:213-274) around Diffusion.sample (gc_diffusion.py:117-216) with the transformer denoiser, on
    a batch: scaled observation window (deque maxlen W; the window GROWS at episode start), ALL L action positions of the window start from noise (no action history,
    unlike BESO), T reverse steps - epsilon prediction, x0 clipped to the data bounds in scaled space, posterior mean, posterior noise except at step 0 -, final clamp,
    the action of the last valid position, inverse scaling.

    Always the fixed-shape form: windows right-padded to W (_History.padded), lengths on the device, in-place history.  Causal attention never lets a valid position see
    the padding behind it and ``pos_emb[:L]`` of the reference equals the first L rows of the padded form, so a lane with L < W entries gets the reference's numbers;
    the few extra tokens during the first W - 1 steps of an episode buy ONE code path that can be captured (CapturedPolicy).

    One predict_batch: the state tokens once (torch), one launch of the step kernel in its init mode (csrc/policy_ddpm_gpt.h through d3il_ddpm_gpt_step_f32: first
    iterate = noise, its action tokens, the time token), then T times the block chain (the last block on the action positions only) and one launch of the step kernel
    (ln_f, head, clipped x0, posterior mean, noise, the next iterate's tokens; at step 0 the clamped, inverse-scaled action), then a device-side add on the step word.

    The noise is Box-Muller on Philox4x32-10 keyed by ``seed`` with counter (env_offset + lane, step word, DDPM_GPT_TAG | k << 8 | j << 1 | q) - chain index k = T for the
    first iterate, i for reverse step i; index 0 is never drawn - so results do not depend on batch order, sub-batches or ranks (``ddpm_gpt_normals`` is the host form);
    or ``noise_in(k, n) -> [n, W, A]`` when given (golden replay, tests).  On the CPU, for unsupported shapes (the Linear-GELU-Linear head among them) and with
    D3IL_POLICY_DDPM_GPT_STEP=0 the same arithmetic runs as torch ops (``_step_torch``) with the Philox normals computed on the host - that path cannot be captured.
    A NaN / Inf in a valid hidden row or iterate marks the environment (``last_bad``) and its action comes out NaN (D3IL_FLAG_SOLVER_FAIL in that lane's step)."""

    def __init__(self, model: DiffusionGPTDenoiser, scaler: Scaler, n_timesteps: int, window_size: int, seed: int = 0, noise_in=None):
        self.model, self.scaler, self.T, self.W = model.eval(), scaler, int(n_timesteps), int(window_size)
        assert 1 <= self.T <= 255 and 1 <= self.W <= 16, "the Philox counter layout holds T <= 255 and W <= 16"
        assert self.W <= model.obs_seq_len, "the window cannot exceed the denoiser's obs_seq_len"
        dev = scaler.x_mean.device
        self.device = dev
        self.A = int(model.action_dim)
        sch = ddpm_schedule(cosine_beta_schedule(self.T).to(dev))
        self.sqrt_recip_ac, self.sqrt_recipm1_ac, self.post_logvar, self.coef1, self.coef2, self._sched = (sch[k] for k in ("sqrt_recip_ac", "sqrt_recipm1_ac", "post_logvar", "coef1", "coef2", "sched"))
        self._init_output(scaler)
        self._init_stream(seed)
        self.noise_in = noise_in
        self.hist = None
        self.record = False           # also keep what every launch drew (last_noise: {k: [n, W, A]})
        self.last_bad = self.last_noise = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, noise_in=None, device=None):
        """From a live reference ``DiffusionAgent`` (duck-typed) whose ``model`` is a ``Diffusion`` around a ``DiffusionTransformerNetwork``: the denoiser's state
        dict, ``n_timesteps``, ``agent.scaler``, ``agent.window_size``; with ``agent.use_ema`` the EMA shadow parameters (the reference swaps them in for every predict)."""
        diff = agent.model
        net = diff.model
        sd = {k: torch.as_tensor(v) for k, v in net.state_dict().items()}
        dev = torch.device(device) if device is not None else sd["tok_emb.weight"].device
        C, state_dim = sd["tok_emb.weight"].shape
        A = sd["action_emb.weight"].shape[1]
        n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        n_heads = int(net.blocks[0].attn.n_head)
        den = DiffusionGPTDenoiser(state_dim, A, C, n_layers, n_heads, sd["pos_emb"].shape[1] - 1, linear_output="action_pred.weight" in sd)
        den.load_state_dict(sd)
        den = den.to(dev).requires_grad_(False)
        pol = cls(den, Scaler.from_reference(agent.scaler, dev), int(diff.n_timesteps), int(agent.window_size), seed=seed, noise_in=noise_in)
        if getattr(agent, "use_ema", False):
            pol.use_ema(agent.ema_helper.shadow_params)
        return pol

    @staticmethod
    def matches(agent) -> bool:
        """Does ``agent`` look like the reference's DiffusionAgent around a DiffusionTransformerNetwork without goals (what from_reference reads), configured as the
        sampler restated here (``model.betas`` = the cosine schedule, epsilon prediction, clip_denoised, neither diffusion_x nor diffusion_kde)?  The DDPM-MLP agent
        (no ``time_emb`` / ``action_emb`` / ``blocks``) and BeT do not."""
        try:
            diff = agent.model
            net = diff.model
            if not (hasattr(net, "time_emb") and hasattr(net, "action_emb") and hasattr(net, "blocks") and hasattr(net, "state_dict") and net.goal_conditioned is False
                    and hasattr(agent, "scaler") and int(agent.window_size) >= 1):
                return False
            # the sampler this policy restates: cosine schedule, epsilon prediction, clipped x0, no diffusion-x tail, no KDE selection - any other switch of the
            # reference's configuration keeps the agent on the row-by-row adapter, which runs the reference's own code
            if getattr(diff, "diffusion_x", False) or getattr(agent, "diffusion_kde", False) or not getattr(diff, "predict_epsilon", True) or not getattr(diff, "clip_denoised", True):
                return False
            T = int(diff.n_timesteps)
            betas = torch.as_tensor(diff.betas).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
            return 1 <= T <= 255 and betas.shape[0] == T and bool(torch.equal(betas, cosine_beta_schedule(T)))
        except (AttributeError, TypeError, ValueError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy)
    SWITCH, LAST, BOUNDS = "D3IL_POLICY_DDPM_GPT_STEP", ("last_bad", "last_noise"), ("min_action", "max_action")

    @property
    def f16x3_blocks(self) -> bool:
        """The blocks run the split-f16 kernels the range guard instruments (CapturedPolicy captures again when the guard changes)."""
        return blocks_f16x3(self.model.blocks)

    def _state(self, n):
        """The observation window for n lanes; a new size starts empty."""
        if self.hist is None or self.hist.buf.shape[0] != n:
            self.hist = _History(n, self.W, self.model.state_dim, self.device)

    def reset(self):
        if self.hist is not None:
            self.hist.reset()

    def begin_episodes(self, mask):
        if self.hist is not None:
            self.hist.reset_(mask)

    def fork(self):
        """A clone for another sub-batch: denoiser, scaler and schedule shared; step word and packed tables its own, an empty history."""
        c = super().fork()
        c.hist = None
        return c

    def load_reference_state_dict(self, sd):
        """``Diffusion.state_dict()`` of the reference: the denoiser sits under ``model.``."""
        self.model.load_state_dict({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")})

    # ---- packed tables
    def _pack_params(self):
        m = self.model
        return list(m.time_emb.parameters()) + [m.action_emb.bias, m.pos_emb]

    def _pack(self):
        """temb [T, C] = time_emb(arange(T)); the schedule table [T, 5] (ddpm_schedule: the one DDPMPolicy packs, sig[0] = 0); bias_pos [W, C] = action_emb.bias + pos_emb[:W]."""
        m, dev = self.model, self.model.pos_emb.device
        return {"temb": m.time_emb(torch.arange(self.T, device=dev)).to(torch.float32).contiguous(),
                "sched": self._sched.to(device=dev, dtype=torch.float32).contiguous(),
                "bias_pos": (m.action_emb.bias + m.pos_emb[0, :self.W]).to(torch.float32).contiguous()}

    def invalidate_packed(self):
        super().invalidate_packed()
        invalidate_blocks_packed(self.model.blocks)

    def ensure_packed(self):
        """The packed tables (on the CPU too: the torch path reads them) and the blocks' packed weights follow the parameters (outside any capture)."""
        self._packed.ensure(self._pack_params(), self._pack)
        if self.model.pos_emb.is_cuda:
            ensure_blocks_packed(self.model.blocks)

    # ---- one step of the chain
    def step_kernel_ok(self, dev) -> bool:
        m = self.model
        C = m.embed_dim
        return (dev.type == "cuda" and m.linear_output and m.pos_emb.dtype == torch.float32 and C <= 128 and C % 4 == 0 and 1 <= self.A <= 8 and 1 <= self.W <= 16 and 1 <= self.T <= 255
                and self._switch_on())

    def _noise(self, k, n, dev):
        """The normals of chain index k as the torch path takes them: ``noise_in(k, n)`` or the host form of the kernel's Philox draw."""
        return self._draw(self.noise_in and (lambda n: self.noise_in(k, n)), n, (n, self.W, self.A),
                          lambda t: ddpm_gpt_normals(self.seed, self.env_offset, n, t, k, self.W, self.A), True, dev)

    def _step_torch(self, st, k, hk):
        """Steps 1 - 8 of csrc/policy_ddpm_gpt.h as torch ops, in the kernel's order of operations, on the chain state ``st`` (x, xbuf, bad, lengths, packed tables)."""
        m, T, W = self.model, self.T, self.W
        x, xbuf, ln, w = st["x"], st["xbuf"], st["len"], st["w"]
        n = x.shape[0]
        valid = (torch.arange(W, device=x.device) < ln.unsqueeze(1)).unsqueeze(2)
        if k == T:
            noise = self._noise(k, n, x.device)
            xp = noise
            st["bad"].zero_()
            hit = ~torch.isfinite(xp)
        else:
            noise = self._noise(k, n, x.device) if (k > 0 or self.noise_in is not None) else torch.zeros_like(x)
            eps = m.action_pred(m.ln_f(hk))
            s = w["sched"][k]
            x0 = torch.minimum(torch.maximum(s[0] * x - s[1] * eps, self.min_action), self.max_action)
            mean = s[2] * x0 + s[3] * x
            xp = mean if k == 0 else mean + s[4] * noise
            hit = ~torch.isfinite(hk).all(dim=2, keepdim=True) | ~torch.isfinite(eps) | ~torch.isfinite(x) | ~torch.isfinite(xp)
        st["bad"] |= (hit & valid).any(dim=2).any(dim=1).to(torch.int32)
        xp = torch.where(valid, xp, torch.zeros_like(xp))
        if self.record:
            self.last_noise[k] = noise
        if k > 0:
            x.copy_(xp)
            xbuf[:, 0] = w["temb"][k - 1]
            xbuf[:, 2::2] = w["bias_pos"] + xp @ m.action_emb.weight.t()
        else:
            last = xp.gather(1, (ln - 1).view(n, 1, 1).expand(-1, 1, self.A)).squeeze(1)
            st["actions"].copy_(self._action_tail(last, st["bad"], False, self.min_action, self.max_action))

    def _step_kernel(self, st, k, hk):
        from . import capi
        m, w, dev = self.model, st["w"], st["x"].device
        n = st["x"].shape[0]
        noise_in = self._noise(k, n, dev) if self.noise_in is not None else None
        noise_out = torch.empty(n, self.W, self.A, dtype=torch.float32, device=dev) if self.record else None
        assert hk is None or hk.is_contiguous()
        assert m.action_pred.weight.is_contiguous() and m.action_emb.weight.is_contiguous()
        capi.launch("d3il_ddpm_gpt_step_f32", dev, hk=hk, ln_weight=m.ln_f.weight, ln_bias=m.ln_f.bias, ln_eps=float(m.ln_f.eps), w_pred=m.action_pred.weight,
                    b_pred=m.action_pred.bias, w_aemb=m.action_emb.weight, bias_pos=w["bias_pos"], temb=w["temb"], sched=w["sched"], **self._draw_args(), len=st["len"],
                    noise_in=noise_in, x=st["x"], xbuf=st["xbuf"], actions=st["actions"], bad=st["bad"], noise_out=noise_out, n_env=n, C=m.embed_dim, A=self.A, W=self.W,
                    T=self.T, k=k)
        if self.record:
            self.last_noise[k] = noise_out

    @torch.no_grad()
    def predict_batch(self, obs):
        s = self.scaler.scale_input(obs.to(device=self.device, dtype=torch.float32))
        m, W, T = self.model, self.W, self.T
        n, dev = s.shape[0], s.device
        if s.is_cuda and not _ENV_GUARD_TRIED and self.f16x3_blocks:
            _env_range_guard(dev)
        if not (s.is_cuda and _capturing()):
            self.ensure_packed()
        assert self._packed.key is not None, "a captured graph replays the packed tables: call ensure_packed() before capturing"
        w = self._packed.buf
        self._state(n)
        self.hist.append_(s)
        states, ln = self.hist.padded()
        C = m.embed_dim
        st = dict(x=torch.empty(n, W, self.A, dtype=torch.float32, device=dev), xbuf=torch.empty(n, 2 * W + 1, C, dtype=torch.float32, device=dev),
                  actions=torch.empty(n, self.A, dtype=torch.float32, device=dev), bad=torch.empty(n, dtype=torch.int32, device=dev), len=ln.contiguous(), w=w)
        # 1. the state tokens: the same in every sampling step
        torch.add(m.tok_emb(states), m.pos_emb[0, :W, :], out=st["xbuf"][:, 1::2])
        if getattr(self, "_keep", None) is None or self._keep.device != dev:
            self._keep = torch.arange(2, 2 * W + 1, 2, device=dev)
        step = self._step_kernel if self.step_kernel_ok(dev) else self._step_torch
        if self.record:
            self.last_noise = {}
        step(st, T, None)                                                    # 2. first iterate = noise, its tokens, the time token of step T - 1
        for i in reversed(range(T)):                                         # 3. T times: the blocks, then everything up to the next token buffer
            step(st, i, m.hidden(st["xbuf"], self._keep).contiguous())
        self._t.add_(1)                                                      # 4. the step word
        self.last_bad = st["bad"]
        return st["actions"]

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, embed_dim: int = 120, n_layers: int = 6, n_heads: int = 6, window_size: int = 5,
               n_timesteps: int = 8, action_scale: float = 0.002, noise_in=None, policy_seed: int = 0, linear_output: bool = True):
        """A policy of the reference's Stacking / Sorting shape (6 layers, 6 heads, 120 wide, window 5, 8 timesteps) with fixed random weights - there are no
        checkpoints offline (as BeTPolicy.random): torch's default layer initialisation, position rows of standard deviation 0.1, a head that predicts noise of
        roughly unit size, unit observation scaling, actions of ``action_scale`` per unit of the scaled space, bounds +-1.5."""
        g = torch.Generator().manual_seed(seed)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            den = DiffusionGPTDenoiser(obs_dim, action_dim, embed_dim, n_layers, n_heads, window_size, linear_output=linear_output)
        with torch.no_grad():
            den.pos_emb.copy_(torch.randn(den.pos_emb.shape, generator=g) * 0.1)
            if linear_output:
                den.action_pred.weight.copy_(torch.randn(den.action_pred.weight.shape, generator=g) * (1.0 / embed_dim ** 0.5))
        return cls(den.requires_grad_(False).to(device), Scaler.unit(obs_dim, action_dim, action_scale, 1.5, device), n_timesteps, window_size, seed=policy_seed, noise_in=noise_in)


# ------------------------------------------------------------------------------------------------ DDPM with the MLP denoiser on the Philox stream
DDPM_MLP_TAG = 0x444D0000     # fourth Philox counter word of the chain kernel, or-ed with k << 1 | q (csrc/policy_ddpm_mlp.h; its upper half is no other tag's)


def ddpm_mlp_words(seed: int, env_offset: int, n: int, t: int, k: int):
    """The Philox words behind ``ddpm_mlp_normals``: uint32 [n, 2 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t,
    DDPM_MLP_TAG | k << 1 | q))."""
    assert 0 <= k <= 254, "the chain draws k = 0 .. T - 1 with T <= 255"
    q, = _tag_axes(2)
    return philox_words(seed, env_offset, n, t, np.uint64(DDPM_MLP_TAG | (k << 1)) | q)


def ddpm_mlp_normals(seed: int, env_offset: int, n: int, t: int, k: int, A: int):
    """The chain kernel's normals of environments 0 .. n-1 at step word t and draw index k (0: the first iterate, 1 + (T - 1 - i): the noise of reverse step i > 0), on
    the host: float64 [n, A].  Exact on the 32-bit words (``ddpm_mlp_words``: two calls q per row) and f64 from there on (``box_muller_f64``); component a = 4 q + m."""
    assert 1 <= A <= 8
    return box_muller_f64(ddpm_mlp_words(seed, env_offset, n, t, k)).reshape(n, 8)[:, :A]


def pack_ddpm_mlp_weights(model: DiffusionMLP, n_timesteps: int) -> dict:
    """The denoiser of a DDPM-MLP policy for k_ddpm_mlp_chain.  The input layer W_in on the row [x (A) | time embedding (t_dim) | state] is split by what its columns
    depend on: ``w_x`` [NT][64][2], the A columns of x packed to 8 in the input-layer order of ``pack_resmlp_weights`` ([T_out][lane (g, i)][s] = W[16 T_out + i][4 s +
    g]); ``w_state`` [NT][64][16], the state columns packed to 64 in the same order; ``tbias`` [T][H] = W_in[:, A : A + t_dim] temb[i] + b_in with ``temb`` [T][t_dim] =
    temp_layers(arange(T)) - the time embedding is the same for every row.  Blocks and output layer as ``pack_resmlp_weights`` packs them."""
    from types import SimpleNamespace
    lin_in, blocks, lin_out = model.layers._parts()
    H, A, td, W = lin_in.out_features, lin_out.out_features, model.temp_layers[-1].out_features, lin_in.weight
    part = lambda a, b: SimpleNamespace(weight=W[:, a:b], bias=lin_in.bias, in_features=b - a, out_features=H)
    pk = pack_resmlp_weights(part(A + td, W.shape[1]), blocks, lin_out, in_cols=64)
    pk["w_state"] = pk.pop("w_in")
    del pk["b_in"]
    pk["w_x"] = pack_resmlp_weights(part(0, A), [], lin_out, in_cols=8)["w_in"]
    f = lambda x: x.detach().to(torch.float32).contiguous()
    pk["temb"] = f(model.temp_layers(torch.arange(n_timesteps, device=W.device)))
    pk["tbias"] = f(pk["temb"] @ W[:, A:A + td].t().to(torch.float32) + lin_in.bias)
    return pk


class DDPMNativePolicy(NativePolicy):
    """DiffusionAgent.predict (agents/ddpm_agent.py:213-274) around Diffusion.sample (gc_diffusion.py:101-216) with the MLP denoiser (diffusion_models.py:20-118 over
    common/mlp.py ResidualMLPNetwork, Mish, not goal conditioned) on a batch, on the Philox stream - BASELINE config 4's policy as a NativePolicy, next to the older
    DDPMPolicy (torch.randn on the device generator, one kernel shape), which bench.py keeps using.  Scale the observation, x = z_0, T reverse steps - eps =
    ResidualMLP([x | temb[i] | s]), x0 = clamp(sra[i] x - srm1[i] eps, lo, hi) in scaled space, x = (c1[i] x0 + c2[i] x) + sig[i] z_k, nothing drawn at i = 0 -, final
    clamp, inverse scaling (product and sum in f32: DDPMGPTPolicy's tail.  The reference's scaler holds f64 statistics, agents/utils/scaler.py:29-36,106-110, so its
    f32 x times f64 std plus f64 mean is an f64 product and sum of the same operands; rounding that to f32 and this tail differ by at most one f32 rounding of
    the product, far inside the reference's own f32 error of the chain).

    No history, whatever ``window_size`` is: the MLP denoiser acts on every window position independently (the reference concatenates [x | t | state] along the last
    axis of a [1, L, .] window and runs Linear layers on it: position l of the output reads position l of the input only), ``Diffusion.sample`` draws one normal per
    position, and DiffusionAgent.predict returns position -1 only (ddpm_agent.py:262-264).  So the action is a function of the NEWEST observation and of the draws of
    the newest position alone; the older positions are computed by the reference and thrown away.  ``window_size >= 1`` is accepted and ignored, ``reset`` and
    ``begin_episodes`` do nothing; tests/golden/ref_ddpm_mlp_agent.npz pins this against the reference at window 5.  (As shipped, DiffusionMLPNetwork.forward raises on
    a window of two or more - it concatenates a [batch, 1, t_dim] time embedding with the [batch, L, .] window, diffusion_models.py:95-104 -, so a live reference agent
    runs this denoiser at window 1 only; the fixture's window case runs the reference with the embedding broadcast over the positions)

    On a HIP device the whole call is ONE kernel (csrc/policy_ddpm_mlp.h through d3il_ddpm_mlp_chain: hidden 128 / 256, 1 <= A <= 8, A + t_dim + obs <= 64 input
    columns, 1 <= T <= 255, any number of blocks), then a device-side add on the step word, so a captured graph draws fresh numbers at every replay.  On the CPU, for
    other shapes and with D3IL_POLICY_DDPM_MLP_CHAIN=0 the same arithmetic in the same order runs as torch ops (``_chain_torch``) with the Philox normals computed
    on the host - that path cannot be captured.  The noise is Box-Muller on Philox4x32-10 keyed by ``seed`` with counter (env_offset + lane, step word,
    DDPM_MLP_TAG | k << 1 | q), k = 0 for z_0 and k = 1 + (T - 1 - i) for reverse step i > 0 - T draws per call -, so results do not depend on batch order,
    sub-batches or ranks (``ddpm_mlp_normals`` is the host form); or ``noise_in(k, n) -> [n, A]`` when given (golden replay, tests).  ``last_bad`` i32 [n] marks
    the environments with a NaN / Inf in their scaled state row, in a draw they use, in an eps or in their final x - their actions are NaN -; with ``record``,
    ``last_noise`` [T + 1, n, A] is what was drawn (the last entry, step i = 0, is zeros)."""

    def __init__(self, model: DiffusionMLP, scaler: Scaler, n_timesteps: int, window_size: int = 1, seed: int = 0, noise_in=None):
        self.model, self.scaler, self.T, self.W = model.eval(), scaler, int(n_timesteps), int(window_size)
        assert 1 <= self.T <= 255, "the Philox counter layout holds T <= 255"
        assert self.W >= 1
        dev = scaler.x_mean.device
        self.device = dev
        lin_in, _, lin_out = model.layers._parts()
        self.A, self.t_dim = int(lin_out.out_features), int(model.temp_layers[-1].out_features)
        self.obs_dim = int(lin_in.in_features) - self.A - self.t_dim
        assert 1 <= self.A <= 8, "the Philox counter layout holds at most 8 action components"
        assert self.obs_dim >= 1, "the denoiser reads [x | time embedding | state]"
        self._sched = ddpm_schedule(cosine_beta_schedule(self.T).to(dev))["sched"]
        self._init_output(scaler)
        self._init_stream(seed)
        self.noise_in = noise_in
        self.record = False           # also keep what the call drew (last_noise)
        self.last_bad = self.last_noise = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, noise_in=None, device=None):
        """From a live reference ``DiffusionAgent`` (duck-typed) whose ``model`` is a ``Diffusion`` around a residual-style ``DiffusionMLPNetwork``: the denoiser's state
        dict (widths and block count read from the keys), ``n_timesteps``, ``agent.scaler``, ``agent.window_size``; with ``agent.use_ema`` the EMA shadow parameters
        (the reference swaps them in for every predict)."""
        diff = agent.model
        sd = {k: torch.as_tensor(v) for k, v in diff.model.state_dict().items()}
        dev = torch.device(device) if device is not None else sd["layers.layers.0.weight"].device
        H, in_dim = sd["layers.layers.0.weight"].shape
        t_dim = sd["temp_layers.3.weight"].shape[0]
        last = max(int(k.split(".")[2]) for k in sd if k.startswith("layers.layers."))
        A = sd["layers.layers.%d.weight" % last].shape[0]
        den = DiffusionMLP(A, in_dim - A - t_dim, t_dim, H, 2 * len({k.split(".")[2] for k in sd if ".l1." in k}))
        den.load_state_dict(sd)
        den = den.to(dev).requires_grad_(False)
        pol = cls(den, Scaler.from_reference(agent.scaler, dev), int(diff.n_timesteps), int(agent.window_size), seed=seed, noise_in=noise_in)
        if getattr(agent, "use_ema", False):
            pol.use_ema(agent.ema_helper.shadow_params)
        return pol

    @staticmethod
    def matches(agent) -> bool:
        """Does ``agent`` look like the reference's DiffusionAgent around a residual-style DiffusionMLPNetwork without goals (``temp_layers`` and ``layers``, none of the
        transformer denoisers' ``time_emb`` / ``action_emb`` / ``blocks`` / ``encoder`` / ``decoder``; plain ``nn.Linear`` layers and Mish blocks without norm, dropout or
        spectral norm; at most 8 action components), configured as the sampler restated here (``model.betas`` = the cosine schedule, epsilon prediction, clip_denoised,
        neither diffusion_x nor diffusion_kde, 1 <= T <= 255)?  Everything else stays on the row-by-row adapter, which runs the reference's own code."""
        try:
            diff = agent.model
            net = diff.model
            if not (hasattr(net, "temp_layers") and hasattr(net, "layers") and hasattr(net, "state_dict")) or any(hasattr(net, k) for k in ("time_emb", "action_emb", "blocks", "encoder", "decoder")):
                return False
            if net.goal_conditioned is not False or not hasattr(agent, "scaler") or agent.scaler.y_bounds is None or int(agent.window_size) < 1:
                return False
            layers, temp = list(net.layers.layers), list(net.temp_layers)
            if not ResidualMLP.is_plain(layers, strict=True) or any(float(getattr(getattr(b, "dropout", None), "p", 0.0)) != 0.0 for b in layers[1:-1]):
                return False
            if len(temp) != 4 or type(temp[1]) is not nn.Linear or not isinstance(temp[2], nn.Mish) or type(temp[3]) is not nn.Linear:
                return False
            A, t_dim = layers[-1].out_features, temp[3].out_features
            if not 1 <= A <= 8 or temp[1].in_features != t_dim or layers[0].in_features - A - t_dim < 1:
                return False
            if getattr(diff, "diffusion_x", False) or getattr(agent, "diffusion_kde", False) or not getattr(diff, "predict_epsilon", True) or not getattr(diff, "clip_denoised", True):
                return False
            T = int(diff.n_timesteps)
            betas = torch.as_tensor(diff.betas).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
            return 1 <= T <= 255 and betas.shape[0] == T and bool(torch.equal(betas, cosine_beta_schedule(T)))
        except (AttributeError, TypeError, ValueError, IndexError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy; no per-lane state: the step word is all a capture puts back)
    SWITCH, LAST, TAKES = "D3IL_POLICY_DDPM_MLP_CHAIN", ("last_bad", "last_noise"), "the denoiser takes %d next to the action and the time embedding"

    def begin_episodes(self, mask):
        pass      # (no history: see the class docstring)

    def load_reference_state_dict(self, sd):
        """``Diffusion.state_dict()`` of the reference: the denoiser sits under ``model.``."""
        self.model.load_state_dict({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")})

    def _pack(self):
        """pack_ddpm_mlp_weights of the denoiser (kernel order, ``temb``, ``tbias``), the schedule table [T, 5] (ddpm_schedule: the one DDPMPolicy packs, sig[0] = 0) and
        the action bounds (lo | hi)."""
        dev = self.model.layers.layers[0].weight.device
        fw = pack_ddpm_mlp_weights(self.model, self.T)
        fw["sched"] = self._sched.to(device=dev, dtype=torch.float32).contiguous()
        fw["bounds"] = torch.cat((self.lo.reshape(-1), self.hi.reshape(-1))).to(device=dev, dtype=torch.float32).contiguous()
        return fw

    def _kernel_shape(self) -> bool:
        lin_in = self.model.layers._parts()[0]
        return lin_in.out_features in (128, 256) and 1 <= self.A <= 8 and lin_in.in_features <= 64 and 1 <= self.T <= 255

    # ---- the chain
    def _noise(self, k, n, dev, need_host: bool):
        """The normals of draw k, [n, A] (``_draw``)."""
        return self._draw(self.noise_in and (lambda n: self.noise_in(k, n)), n, (n, self.A), lambda t: ddpm_mlp_normals(self.seed, self.env_offset, n, t, k, self.A), need_host, dev)

    def _chain_torch(self, s, noise):
        """Steps 1 - 3 of csrc/policy_ddpm_mlp.h as torch ops in the dtype of ``s`` (f32 in the policy), in the kernel's order of operations - the input layer as
        (time share + x share) + state share - on the draws ``noise`` [T, n, A]: returns (actions, bad)."""
        dt, dev, A, td = s.dtype, s.device, self.A, self.t_dim
        m = self.model
        lin_in, blocks, lin_out = m.layers._parts()
        c = lambda p: p.to(device=dev, dtype=dt)
        W, noise = c(lin_in.weight), c(noise)
        tbias = c(m.temp_layers(torch.arange(self.T, device=lin_in.weight.device))) @ W[:, A:A + td].t() + c(lin_in.bias)
        xs = s @ W[:, A + td:].t()
        sched, lo, hi = c(self._sched), c(self.lo), c(self.hi)
        x = noise[0]
        bad = ~torch.isfinite(s).all(dim=1) | ~torch.isfinite(x).all(dim=1)
        for step in range(self.T):
            i = self.T - 1 - step
            h = (tbias[i] + x @ W[:, :A].t()) + xs
            for l1, l2 in blocks:
                h = h + F.linear(F.mish(F.linear(F.mish(h), c(l1.weight), c(l1.bias))), c(l2.weight), c(l2.bias))
            eps = F.linear(h, c(lin_out.weight), c(lin_out.bias))
            sc = sched[i]
            x0 = torch.minimum(torch.maximum(sc[0] * x - sc[1] * eps, lo), hi)
            x = sc[2] * x0 + sc[3] * x
            bad |= ~torch.isfinite(eps).all(dim=1)
            if i > 0:
                z = noise[step + 1]
                bad |= ~torch.isfinite(z).all(dim=1)
                x = x + sc[4] * z
        bad |= ~torch.isfinite(x).all(dim=1)
        return self._action_tail(x, bad, False, self.lo, self.hi), bad

    def _step_torch(self, s):
        n, dev = s.shape[0], s.device
        noise = torch.stack([self._noise(k, n, dev, True) for k in range(self.T)])
        y, bad = self._chain_torch(s, noise)
        self.last_bad = bad.to(torch.int32)
        self.last_noise = torch.cat((noise, torch.zeros_like(noise[:1]))) if self.record else None
        return y

    def _step_kernel(self, s):
        from . import capi
        n, dev = s.shape[0], s.device
        w = self._packed.current(self._pack_params(), self._pack)
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        bad = torch.empty(n, dtype=torch.int32, device=dev)
        noise_in = torch.stack([self._noise(k, n, dev, False) for k in range(self.T)]).contiguous() if self.noise_in is not None else None
        noise_out = torch.empty(self.T + 1, n, self.A, dtype=torch.float32, device=dev) if self.record else None
        lin_in, blocks, _ = self.model.layers._parts()
        capi.launch("d3il_ddpm_mlp_chain", dev, state=s, w_x=w["w_x"], w_state=w["w_state"], tbias=w["tbias"], w_blocks=w["w_blk"], b_blocks=w["b_blk"], w_out=w["w_out"],
                    b_out=w["b_out"], sched=w["sched"], **self._draw_args(), noise_in=noise_in, actions=y, bad=bad, noise_out=noise_out, n_env=n, obs_dim=self.obs_dim,
                    A=self.A, t_dim=self.t_dim, n_timesteps=self.T, hidden=lin_in.out_features, n_blocks=len(blocks))
        self.last_bad, self.last_noise = bad, noise_out
        return y

    def _fallback_text(self):
        lin_in = self.model.layers._parts()[0]
        return ("this denoiser (hidden %d, %d input columns, %d action components, %d timesteps) is not one the chain kernel is built for; every call runs torch's "
                "layers with the Philox numbers drawn on the host (a device synchronisation per call, no graph capture)" % (lin_in.out_features, lin_in.in_features, self.A, self.T))

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, hidden_dim: int = 256, n_blocks: int = 4, t_dim: int = 8, n_timesteps: int = 4,
               window_size: int = 1, action_scale: float = 0.002, policy_seed: int = 0, bound: float = 1.5, noise_in=None):
        """A policy of the reference's shape with fixed random weights (there are no checkpoints offline; the defaults are Sorting-4: hidden 256, 8 hidden layers, t_dim
        8, 4 timesteps): torch's default layer initialisation under ``seed`` (the global generator is left alone), unit observation scaling, actions of
        ``action_scale`` per unit of the scaled space, bounds +-``bound``."""
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            den = DiffusionMLP(action_dim, obs_dim, t_dim, hidden_dim, 2 * n_blocks)
        return cls(den.requires_grad_(False).to(device), Scaler.unit(obs_dim, action_dim, action_scale, bound, device), n_timesteps, window_size, seed=policy_seed, noise_in=noise_in)


# ------------------------------------------------------------------------------------------------ BESO on the Philox stream
BESO_TAG = 0x42530000        # fourth Philox counter word of the step kernel, or-ed with draw << 8 | j << 1 | q (csrc/policy_beso.h; its upper half is no other tag's)


def beso_words(seed: int, env_offset: int, n: int, t: int, d: int, W: int):
    """The Philox words behind ``beso_normals``: uint32 [n, W, 2 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t,
    BESO_TAG | d << 8 | j << 1 | q)).  Draw index d = 0 is the init draw (the kernel takes j = 0 only), d = i + 1 the draw of sampling step i."""
    assert 0 <= d <= 254 and 1 <= W <= 16, "the counter layout holds d <= 254 and j <= 15"
    j, q = _tag_axes(W, 2)
    return philox_words(seed, env_offset, n, t, np.uint64(BESO_TAG | (d << 8)) | (j << np.uint64(1)) | q)


def beso_normals(seed: int, env_offset: int, n: int, t: int, d: int, W: int, A: int):
    """The step kernel's normals of environments 0 .. n-1 at step word t and draw index d, on the host: float64 [n, W, A].  Exact on the 32-bit words
    (``beso_words``: two calls q per (row, j)) and f64 from there on (``box_muller_f64``); component a = 4 q + m.  Of d = 0 the sampler uses row j = 0 only."""
    assert 1 <= A <= 8
    return box_muller_f64(beso_words(seed, env_offset, n, t, d, W)).reshape(n, W, 8)[:, :, :A]


def beso_coefficients(sigmas, sigma_data: float):
    """The per-step constants of the sampler from the noise levels ``sigmas`` (S + 1 host floats: the f32 schedule, last entry 0), computed in f64: rows i < S of
    (c_skip, c_out, 1 / s_from, s_down - s_from, s_up, c_in of sigmas[i + 1]) - GCDenoiser.get_scalings (score_wrappers.py:31-43) and get_ancestral_step
    (gc_sampling.py:107-114) with eta = 1 - and c_in of sigmas[0].  The last row's c_in is 0: there is no next iterate."""
    sd2 = float(sigma_data) ** 2
    c_in = lambda sg: 1.0 / (sg ** 2 + sd2) ** 0.5
    rows = []
    for i in range(len(sigmas) - 1):
        s_from, s_to = float(sigmas[i]), float(sigmas[i + 1])
        s_up = min(s_to, (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5)
        s_down = (s_to ** 2 - s_up ** 2) ** 0.5
        rows.append([sd2 / (s_from ** 2 + sd2), s_from * sigma_data / (s_from ** 2 + sd2) ** 0.5, 1.0 / s_from, s_down - s_from, s_up, c_in(s_to) if i + 2 < len(sigmas) else 0.0])
    return rows, c_in(float(sigmas[0]))


class BESONativePolicy(NativePolicy):
    """BesoAgent.predict (beso_agent.py:316-443) with the euler_ancestral sampler on the linear noise schedule (gc_sampling.py:41-44, 107-114, 217-256) around the
    Karras-preconditioned DiffusionGPT (score_wrappers.py GCDenoiser), on a batch and on the Philox stream - what BESOPolicy computes, as a NativePolicy: scaled
    observation window (deque maxlen W), the previous W - 1 clamped scaled actions as the first iterate's earlier positions, sigma_max noise at the newest one, S
    sampling steps over ALL positions, final clamp of the newest position, inverse scaling.

    Always the fixed-shape form (as DDPMGPTPolicy): windows right-padded to W (_History.padded), lengths on the device, in-place histories - ONE code path that
    CapturedPolicy can capture.  The action ring ``a_hist`` [N, W - 1, A] (newest entry last) is per-lane device state the kernel reads and pushes in place.

    One predict_batch: the state tokens once (torch), one launch of the step kernel in its init mode (csrc/policy_beso.h through d3il_beso_step: first iterate, its
    action tokens, the sigma token), then S times the block chain (the last block on the action positions only) and one launch of the step kernel (ln_f, head,
    Karras combination, Euler step, ancestral noise, the next iterate's tokens; at step S - 1 the clamped, inverse-scaled action and the ring push), then a
    device-side add on the step word.  The arithmetic follows the reference's order step by step (not the merged form of BESOPolicy._sample_device).

    The noise is Box-Muller on Philox4x32-10 keyed by ``seed`` with counter (env_offset + lane, step word, BESO_TAG | d << 8 | j << 1 | q) - draw index d = 0 (j = 0)
    for the init draw, d = i + 1 for sampling step i; the last step draws nothing - so results do not depend on batch order, sub-batches or ranks (``beso_normals`` is
    the host form); or ``noise_in(d, n) -> [n, W, A]`` when given (golden replay, tests; of d = 0 row j = 0 is used).  On the CPU, for unsupported shapes (the
    Linear-SiLU-Linear head among them) and with D3IL_POLICY_BESO_STEP=0 the same arithmetic runs as torch ops (``_step_torch``) with the Philox normals computed
    on the host - that path cannot be captured.  A NaN / Inf in a valid hidden row or iterate marks the environment (``last_bad``): its action and the ring entry it
    pushes come out NaN (D3IL_FLAG_SOLVER_FAIL in that lane's step)."""

    def __init__(self, model: DiffusionGPT, scaler: Scaler, window_size: int, num_sampling_steps: int, sigma_min: float, sigma_max: float, sigma_data: float = 0.5,
                 seed: int = 0, noise_in=None):
        self.model, self.scaler, self.W, self.S = model.eval(), scaler, int(window_size), int(num_sampling_steps)
        assert 1 <= self.S <= 254 and 1 <= self.W <= 16, "the Philox counter layout holds S <= 254 and W <= 16"
        assert self.W <= model.obs_seq_len, "the window cannot exceed the network's obs_seq_len"
        dev = scaler.x_mean.device
        self.device = dev
        self.A, self.obs_dim = int(model.action_emb.in_features), int(model.tok_emb.in_features)
        self.sigma_min, self.sigma_max, self.sigma_data = float(sigma_min), float(sigma_max), float(sigma_data)
        # the noise schedule as host floats of its f32 values (as BESOPolicy.sigmas) and the constants derived from them
        self.sigmas = torch.cat([torch.linspace(self.sigma_max, self.sigma_min, self.S), torch.zeros(1)]).tolist()
        self._coef, self.c_in0 = beso_coefficients(self.sigmas, self.sigma_data)
        self._init_output(scaler)
        self._init_stream(seed)
        self.noise_in = noise_in
        self.hist = self.a_hist = None
        self.record = False           # also keep what every launch drew (last_noise: {d: [n, W, A]})
        self.last_bad = self.last_noise = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, noise_in=None, device=None):
        """From a live reference ``BesoAgent`` (duck-typed) whose ``model`` is a ``GCDenoiser`` around a ``DiffusionGPT``: the network's state dict, the sampler's
        settings, ``agent.scaler``, ``agent.window_size``; with ``agent.use_ema`` the EMA shadow parameters (the reference swaps them in for every predict)."""
        net = agent.model.inner_model
        sd = {k: torch.as_tensor(v) for k, v in net.state_dict().items()}
        dev = torch.device(device) if device is not None else sd["tok_emb.weight"].device
        C, state_dim = sd["tok_emb.weight"].shape
        A = sd["action_emb.weight"].shape[1]
        n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        n_heads = int(net.blocks[0].attn.n_head)
        own = DiffusionGPT(state_dim, A, C, n_layers, n_heads, sd["pos_emb"].shape[1] - 1, linear_output="action_pred.weight" in sd)
        keys = own.state_dict()
        own.load_state_dict({k: v for k, v in sd.items() if k in keys})
        own = own.to(dev).requires_grad_(False)
        pol = cls(own, Scaler.from_reference(agent.scaler, dev), int(agent.window_size), int(agent.num_sampling_steps), float(agent.sigma_min), float(agent.sigma_max),
                  sigma_data=float(agent.sigma_data), seed=seed, noise_in=noise_in)
        if getattr(agent, "use_ema", False):
            pol.use_ema(agent.ema_helper.shadow_params)
        return pol

    @staticmethod
    def matches(agent) -> bool:
        """Does ``agent`` look like the reference's BesoAgent around GCDenoiser(DiffusionGPT) without goals (what from_reference reads), configured as the sampler
        restated here: ``sampler_type`` euler_ancestral, ``noise_scheduler`` linear, a linear or Linear-SiLU-Linear head?  Any other setting keeps the agent on the
        row-by-row adapter, which runs the reference's own code."""
        try:
            net = agent.model.inner_model
            if not (hasattr(agent.model, "get_scalings") and hasattr(net, "sigma_emb") and hasattr(net, "action_emb") and hasattr(net, "blocks") and hasattr(net, "state_dict")
                    and net.goal_conditioned is False and not getattr(agent, "gc", False) and hasattr(agent, "scaler") and hasattr(agent, "action_context")):
                return False
            if agent.sampler_type != "euler_ancestral" or agent.noise_scheduler != "linear":
                return False
            head = net.action_pred
            if not (isinstance(head, nn.Linear) or (isinstance(head, nn.Sequential) and len(head) == 3 and isinstance(head[0], nn.Linear) and isinstance(head[1], nn.SiLU)
                                                    and isinstance(head[2], nn.Linear))):
                return False
            W, S = int(agent.window_size), int(agent.num_sampling_steps)
            return 1 <= W <= min(16, int(net.pos_emb.shape[1]) - 1) and 1 <= S <= 254 and float(agent.sigma_max) >= float(agent.sigma_min) > 0.0
        except (AttributeError, TypeError, ValueError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy)
    SWITCH, STATE, LAST, BOUNDS = "D3IL_POLICY_BESO_STEP", ("a_hist",), ("last_bad", "last_noise"), ("min_action", "max_action")

    @property
    def f16x3_blocks(self) -> bool:
        """The blocks run the split-f16 kernels the range guard instruments (CapturedPolicy captures again when the guard changes)."""
        return blocks_f16x3(self.model.blocks)

    def weights_out_of_range(self) -> int:
        """As BESOPolicy.weights_out_of_range: entries of the blocks' f16x3-packed matrices that are NaN / Inf or beyond +-65504; one synchronising read."""
        return blocks_w_oor(self.model.blocks)

    def range_report(self) -> dict:
        """The active RangeGuard's counters (clipped / nonfinite / launches) plus ``weights_out_of_range``."""
        g = range_guard()
        if g is None:
            raise RuntimeError("range_report: no RangeGuard is enabled (policies.RangeGuard, D3IL_POLICY_RANGE_GUARD=1 or a Sim's policy_range_guard=True)")
        rep = g.read()
        rep["weights_out_of_range"] = self.weights_out_of_range()
        return rep

    def _state(self, n):
        """The observation window and the action ring for n lanes; a new size starts empty."""
        if self.hist is None or self.hist.buf.shape[0] != n:
            self.hist = _History(n, self.W, self.obs_dim, self.device)
            self.a_hist = torch.zeros(n, self.W - 1, self.A, dtype=torch.float32, device=self.device)

    def reset(self):
        if self.hist is not None:
            self.hist.reset()

    def begin_episodes(self, mask):
        """Lanes that start a new trajectory: window length 0 (in place).  Their ring entries are not read again before they are overwritten."""
        if self.hist is not None:
            self.hist.reset_(mask)

    def fork(self):
        """A clone for another sub-batch: network, scaler and schedule shared; step word and packed tables its own, empty histories."""
        c = super().fork()
        c.hist = c.a_hist = None
        return c

    def load_reference_state_dict(self, sd):
        """``GCDenoiser.state_dict()`` of the reference: the transformer sits under ``inner_model.``."""
        own = self.model.state_dict()
        self.model.load_state_dict({k[len("inner_model."):]: v for k, v in sd.items() if k.startswith("inner_model.") and k[len("inner_model."):] in own})

    # ---- packed tables
    def _pack_params(self):
        m = self.model
        return list(m.sigma_emb.parameters()) + [m.action_emb.bias, m.pos_emb]

    def _pack(self):
        """semb [S, C] = sigma_emb(log(sigma) / 4) of the S noise levels; coef [S, 6] (beso_coefficients); bias_pos [W, C] = action_emb.bias + pos_emb[:W]."""
        m, dev = self.model, self.model.pos_emb.device
        sig = torch.tensor(self.sigmas[:-1], dtype=torch.float32, device=dev)
        return {"semb": m.sigma_emb(sig.reshape(-1, 1).log() / 4).to(torch.float32).contiguous(),
                "coef": torch.tensor(self._coef, dtype=torch.float64).to(device=dev, dtype=torch.float32).contiguous(),
                "bias_pos": (m.action_emb.bias + m.pos_emb[0, :self.W]).to(torch.float32).contiguous()}

    def invalidate_packed(self):
        super().invalidate_packed()
        invalidate_blocks_packed(self.model.blocks)

    def ensure_packed(self):
        """The packed tables (on the CPU too: the torch path reads them) and the blocks' packed weights follow the parameters (outside any capture)."""
        self._packed.ensure(self._pack_params(), self._pack)
        if self.model.pos_emb.is_cuda:
            ensure_blocks_packed(self.model.blocks)

    # ---- one step of the chain
    def step_kernel_ok(self, dev) -> bool:
        m = self.model
        C = m.embed_dim
        return (dev.type == "cuda" and isinstance(m.action_pred, nn.Linear) and m.pos_emb.dtype == torch.float32 and C <= 128 and C % 4 == 0 and 1 <= self.A <= 8
                and 1 <= self.W <= 16 and 1 <= self.S <= 254 and self._switch_on())

    def _noise(self, d, n, dev):
        """The normals of draw index d as the torch path takes them: ``noise_in(d, n)`` or the host form of the kernel's Philox draw."""
        return self._draw(self.noise_in and (lambda n: self.noise_in(d, n)), n, (n, self.W, self.A),
                          lambda t: beso_normals(self.seed, self.env_offset, n, t, d, self.W, self.A), True, dev)

    def _step_torch(self, st, i, hk):
        """Steps 1 - 8 of csrc/policy_beso.h as torch ops, in the kernel's order of operations, on the chain state ``st`` (x, xbuf, bad, lengths, packed tables)."""
        m, S, W, A = self.model, self.S, self.W, self.A
        x, xbuf, w = st["x"], st["xbuf"], st["w"]
        n = x.shape[0]
        ln = st["len"].clamp(1, W)
        jj = torch.arange(W, device=x.device)
        valid = (jj < ln.unsqueeze(1)).unsqueeze(2)
        last = i == S - 1
        if i < 0:
            nz = self._noise(0, n, x.device)
            noise = torch.zeros_like(x)
            noise[:, 0] = nz[:, 0]
            xp = torch.where((jj == (ln - 1).unsqueeze(1)).unsqueeze(2), (self.sigma_max * nz[:, :1]).expand(-1, W, -1), torch.zeros_like(x))
            if W > 1:
                src = ((W - 1) - (ln - 1)).unsqueeze(1) + jj
                prev = torch.gather(self.a_hist, 1, src.clamp(0, W - 2).unsqueeze(2).expand(-1, -1, A))
                xp = torch.where((jj < (ln - 1).unsqueeze(1)).unsqueeze(2), prev, xp)
            st["bad"].zero_()
            hit = ~torch.isfinite(xp)
            c_in = self.c_in0
        else:
            noise = torch.zeros_like(x) if last else self._noise(i + 1, n, x.device)
            net = m.action_pred(m.ln_f(hk))
            c = w["coef"][i]
            den = c[1] * net + c[0] * x
            d = (x - den) * c[2]
            xp = x + d * c[3]
            if not last:
                xp = xp + c[4] * noise
            hit = ~torch.isfinite(hk).all(dim=2, keepdim=True) | ~torch.isfinite(net) | ~torch.isfinite(x) | ~torch.isfinite(xp)
            c_in = c[5]
        st["bad"] |= (hit & valid).any(dim=2).any(dim=1).to(torch.int32)
        xp = torch.where(valid, xp, torch.zeros_like(xp))
        if self.record:
            self.last_noise[i + 1] = noise
        if not last:
            x.copy_(xp)
            xbuf[:, 0] = w["semb"][i + 1]
            xbuf[:, 2::2] = w["bias_pos"] + (c_in * xp) @ m.action_emb.weight.t()
        else:
            newest = xp.gather(1, (ln - 1).view(n, 1, 1).expand(-1, 1, A)).squeeze(1)
            a_new = torch.minimum(torch.maximum(newest, self.min_action), self.max_action)
            a_new = torch.where(st["bad"].bool().unsqueeze(1), torch.full_like(a_new, float("nan")), a_new)
            st["actions"].copy_(self._action_tail(a_new, st["bad"], False))
            if W > 1:
                self.a_hist[:, :-1] = self.a_hist[:, 1:].clone()
                self.a_hist[:, -1] = a_new

    def _step_kernel(self, st, i, hk):
        from . import capi
        m, w, dev = self.model, st["w"], st["x"].device
        n = st["x"].shape[0]
        noise_in = self._noise(i + 1, n, dev) if (self.noise_in is not None and i < self.S - 1) else None
        noise_out = torch.empty(n, self.W, self.A, dtype=torch.float32, device=dev) if self.record else None
        assert hk is None or hk.is_contiguous()
        assert m.action_pred.weight.is_contiguous() and m.action_emb.weight.is_contiguous() and self.a_hist.is_contiguous()
        capi.launch("d3il_beso_step", dev, hk=hk, ln_weight=m.ln_f.weight, ln_bias=m.ln_f.bias, ln_eps=float(m.ln_f.eps), w_pred=m.action_pred.weight,
                    b_pred=m.action_pred.bias, w_aemb=m.action_emb.weight, bias_pos=w["bias_pos"], semb=w["semb"], coef=w["coef"], sigma_max=self.sigma_max,
                    c_in0=self.c_in0, **self._draw_args(), len=st["len"], noise_in=noise_in, x=st["x"], xbuf=st["xbuf"], a_hist=self.a_hist if self.W > 1 else None,
                    actions=st["actions"], bad=st["bad"], noise_out=noise_out, n_env=n, C=m.embed_dim, A=self.A, W=self.W, S=self.S, i=i)
        if self.record:
            self.last_noise[i + 1] = noise_out

    @torch.no_grad()
    def predict_batch(self, obs):
        s = self.scaler.scale_input(obs.to(device=self.device, dtype=torch.float32))
        assert s.dim() == 2 and s.shape[1] == self.obs_dim, "BESONativePolicy: observation width %d, the network takes %d" % (s.shape[-1], self.obs_dim)
        m, W, S = self.model, self.W, self.S
        n, dev = s.shape[0], s.device
        if s.is_cuda and not _ENV_GUARD_TRIED and self.f16x3_blocks:
            _env_range_guard(dev)
        if not (s.is_cuda and _capturing()):
            self.ensure_packed()
        assert self._packed.key is not None, "a captured graph replays the packed tables: call ensure_packed() before capturing"
        w = self._packed.buf
        self._state(n)
        self.hist.append_(s)
        states, ln = self.hist.padded()
        C = m.embed_dim
        st = dict(x=torch.empty(n, W, self.A, dtype=torch.float32, device=dev), xbuf=torch.empty(n, 2 * W + 1, C, dtype=torch.float32, device=dev),
                  actions=torch.empty(n, self.A, dtype=torch.float32, device=dev), bad=torch.empty(n, dtype=torch.int32, device=dev), len=ln.contiguous(), w=w)
        # 1. the state tokens: the same in every sampling step
        torch.add(m.tok_emb(states), m.pos_emb[0, :W, :], out=st["xbuf"][:, 1::2])
        if getattr(self, "_keep", None) is None or self._keep.device != dev:
            self._keep = torch.arange(2, 2 * W + 1, 2, device=dev)
        kernel = self.step_kernel_ok(dev)
        if not kernel:
            self._warn_fallback(s, lambda: "the step kernel is built for a linear head, n_embd <= 128 (a multiple of 4), 1 .. 8 action components, a window of 1 .. 16: torch glue")
        step = self._step_kernel if kernel else self._step_torch
        if self.record:
            self.last_noise = {}
        step(st, -1, None)                                                   # 2. the first iterate, its tokens, the sigma token of step 0
        for i in range(S):                                                   # 3. S times: the blocks, then everything up to the next token buffer
            step(st, i, m.hidden(st["xbuf"], self._keep).contiguous())
        self._t.add_(1)                                                      # 4. the step word
        self.last_bad = st["bad"]
        return st["actions"]

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, embed_dim: int = 120, n_layers: int = 6, n_heads: int = 6, window_size: int = 5,
               num_sampling_steps: int = 16, sigma_min: float = 0.01, sigma_max: float = 1.0, action_scale: float = 0.002, noise_in=None, policy_seed: int = 0,
               linear_output: bool = True):
        """A policy of the reference's Stacking shape (6 layers, 6 heads, 120 wide, window 5, 16 sampling steps, sigma 0.01 .. 1) with fixed random weights - there
        are no checkpoints offline (as DDPMGPTPolicy.random): torch's default layer initialisation, position rows of standard deviation 0.1, a head of roughly unit
        output, unit observation scaling, actions of ``action_scale`` per unit of the scaled space, bounds +-1.5."""
        g = torch.Generator().manual_seed(seed)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            net = DiffusionGPT(obs_dim, action_dim, embed_dim, n_layers, n_heads, window_size, linear_output=linear_output)
        with torch.no_grad():
            net.pos_emb.copy_(torch.randn(net.pos_emb.shape, generator=g) * 0.1)
            if linear_output:
                net.action_pred.weight.copy_(torch.randn(net.action_pred.weight.shape, generator=g) * (1.0 / embed_dim ** 0.5))
        return cls(net.requires_grad_(False).to(device), Scaler.unit(obs_dim, action_dim, action_scale, 1.5, device), window_size, num_sampling_steps, sigma_min, sigma_max,
                   seed=policy_seed, noise_in=noise_in)


# ------------------------------------------------------------------------------------------------ Implicit BC: Langevin chain on an energy network
IBC_TAG = 0x49420000          # fourth Philox counter word of the chain kernel, or-ed with kind << 14 | k << 8 | s << 2 | q (csrc/policy_ibc.h; never 0, BET_TAG or a DDPM_GPT_TAG word)
IBC_EDGE = 1e-4               # a draw this close to an edge of the normalised CDF is not decided between two arithmetics (tests, golden generator)


def ibc_words(seed: int, env_offset: int, n: int, t: int, kind: int, k: int, S: int = 64):
    """The Philox words of the chain kernel: uint32 [n, S, 2 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t,
    IBC_TAG | kind << 14 | k << 8 | s << 2 | q)); kind 0 = start point, 1 = noise of iteration k, 2 = the draw (s = q = 0 is the word that is used)."""
    assert 0 <= kind <= 2 and 0 <= k <= 63 and 1 <= S <= 64, "the counter layout holds k <= 63 and s <= 63"
    s, q = _tag_axes(S, 2)
    return philox_words(seed, env_offset, n, t, np.uint64(IBC_TAG | (kind << 14) | (k << 8)) | (s << np.uint64(2)) | q)


def ibc_start_uniforms(seed: int, env_offset: int, n: int, t: int, A: int, S: int = 64):
    """The kernel's start-point uniforms of environments 0 .. n-1 at step word t: float32 [n, S, A] in [0, 1 - 2^-24], component a = 4 q + m takes word m of
    call q.  The start point is lo + u (hi - lo), every operation rounded to f32."""
    assert 1 <= A <= 8
    return uniform24(ibc_words(seed, env_offset, n, t, 0, 0, S).reshape(n, S, 8)[:, :, :A])


def ibc_normals(seed: int, env_offset: int, n: int, t: int, k: int, A: int, S: int = 64):
    """The kernel's normals of iteration k: float64 [n, S, A].  Exact on the words and f64 from there on (``box_muller_f64``)."""
    assert 1 <= A <= 8
    return box_muller_f64(ibc_words(seed, env_offset, n, t, 1, k, S)).reshape(n, S, 8)[:, :, :A]


def ibc_pick_uniforms(seed: int, env_offset: int, n: int, t: int):
    """The kernel's uniform of the categorical draw, one per environment: float32 [n]."""
    return uniform24(ibc_words(seed, env_offset, n, t, 2, 0, 1)[:, 0, 0, 0])


def ibc_step_sizes(iterations: int, init_infer: float, init: float, final: float, power: float, second_init: float, second: bool = True):
    """The step sizes of LangevinMCMCSampler.infer as Python floats: the first step is ``sampler_stepsize_init_infer``, steps 1 .. I-1 follow the polynomial
    schedule that starts from ``sampler_stepsize_init`` (NOT the _infer value; schedulers.py:16-23 with its I - 1 denominator), the second loop of I steps
    keeps ``second_inference_stepsize_init``."""
    I = int(iterations)
    steps = [float(init_infer)] + [(init - final) * ((1.0 - float(i) / float(I - 1)) ** power) + final for i in range(1, I)]
    return steps[:I] + ([float(second_init)] * I if second else [])


def _mish_and_derivative(x):
    """Mish and its derivative in the form of csrc/policy_ibc.h ibc_mish: n = e^x, p = n (n + 2), t = p / (p + 2); x t and t + x 4 n (n + 1) / (p + 2)^2; x > 20: x, 1."""
    big = x > 20.0
    n = torch.exp(torch.where(big, torch.zeros_like(x), x))
    p = n * (n + 2.0)
    q = p + 2.0
    t = p / q
    return torch.where(big, x, x * t), torch.where(big, torch.ones_like(x), t + x * (4.0 * n * (n + 1.0)) / (q * q))


def resmlp_energy_and_grad(model: ResidualMLP, rows, obs_dim: int, grad: bool = True):
    """E = model(rows)[:, 0] and dE / d rows[:, obs_dim:] of a ResidualMLP with one output, analytically, in the dtype of ``rows`` and the parameters:
    per block y = x + W2 m(W1 m(x) + b1) + b2 the row gradient is gx = gy + m'(x) . ((m'(u) . (gy W2)) W1); the chain starts from the output row."""
    lin_in, blocks, lin_out = model._parts()
    x = F.linear(rows, lin_in.weight, lin_in.bias)
    kept = []
    for l1, l2 in blocks:
        m0, d0 = _mish_and_derivative(x)
        m1, d1 = _mish_and_derivative(F.linear(m0, l1.weight, l1.bias))
        x = x + F.linear(m1, l2.weight, l2.bias)
        kept.append((d0, d1))
    e = F.linear(x, lin_out.weight, lin_out.bias)[:, 0]
    if not grad:
        return e, None
    g = lin_out.weight[0].expand_as(x)
    for (l1, l2), (d0, d1) in zip(reversed(blocks), reversed(kept)):
        g = g + d0 * ((d1 * (g @ l2.weight)) @ l1.weight)
    return e, g @ lin_in.weight[:, obs_dim:]


class IBCPolicy(NativePolicy):
    """IBCAgent.predict without goals (agents/ibc_agent.py:248-286) around LangevinMCMCSampler.infer (samplers/langevin_mcmc.py:129-163, 236-286) on the energy
    network EBMMLP (ebms.py:21-51: a ResidualMLPNetwork on [state | action] with one output), on a batch: scale the observation, S uniform start points per
    environment inside the data bounds (scaled space), K Langevin iterations x <- clamp(x - clamp(step / 2 dE/dx + step noise_scale z, +-clip), lo, hi) with
    clip = delta_action_clip (hi - lo) / 2 - the noise is multiplied by the step, not by its root, as the reference does; the samples are carried in f64 and the
    network runs in f32, also as the reference does (its f64 bounds array promotes the samples, ResidualMLPNetwork.forward casts to f32) -, one categorical draw from
    softmax(-E) of the final samples, inverse scaling (no clamp afterwards: the sampler's bounds are the only one).  ``steps`` is the table of
    ``ibc_step_sizes``.

    On a HIP device the whole call is ONE kernel (csrc/policy_ibc.h through d3il_ibc_langevin_f32: forward pass, analytic backward pass and update for all
    iterations, the energies and the draw; hidden 128 / 256, at most 4 blocks, obs + A <= 28, S = 64, K <= 63), then a device-side add on the step word.  On the
    CPU, for other shapes and with D3IL_POLICY_IBC_FUSED=0 the same arithmetic runs as torch ops (``_chain_torch``, the analytic gradient of
    ``resmlp_energy_and_grad``) on the same Philox stream computed on the host - that path cannot be captured.  Random numbers: Philox4x32-10 keyed by ``seed``
    with counter (env_offset + lane, step word, IBC_TAG | kind << 14 | k << 8 | s << 2 | q), so results do not depend on batch order, sub-batches or ranks;
    ``x0_in(n) -> [n, S, A]``, ``noise_in(n) -> [K, n, S, A]`` (standard normals) and ``u_in(n) -> [n]`` replace the draws when given (golden replay, tests).
    A NaN / Inf in an environment's state row, iterates or final energies gives that environment a NaN action (``last_picks`` = -1)."""

    def __init__(self, model: ResidualMLP, scaler: Scaler, steps, noise_scale: float = 0.5, delta_action_clip: float = 0.1, samples: int = 64, seed: int = 0,
                 n_envs: int | None = None, bounds=None, x0_in=None, noise_in=None, u_in=None):
        self.model, self.scaler = model.eval(), scaler
        dev = scaler.x_mean.device
        self.device = dev
        lin_in, _, lin_out = model._parts()
        assert lin_out.out_features == 1, "the energy network has one output"
        b = torch.as_tensor(scaler.y_bounds if bounds is None else bounds).detach().to(device="cpu", dtype=torch.float64)
        self.A = int(b.shape[1])
        self.obs_dim = int(lin_in.in_features) - self.A
        self.S, self.K = int(samples), len(steps)
        assert 1 <= self.A <= 8 and 1 <= self.S <= 64 and 0 <= self.K <= 63, "the Philox counter layout holds A <= 8, S <= 64 and K <= 63"
        self.steps = [float(v) for v in steps]
        self.noise_scale, self.delta_action_clip = float(noise_scale), float(delta_action_clip)
        f = lambda a: a.to(device=dev, dtype=torch.float32).contiguous()
        self._init_output(scaler, b[0], b[1])
        self.clip = f(self.delta_action_clip * 0.5 * (b[1] - b[0]))      # (the clip in f64 from the f64 bounds, as the reference)
        self.coef = f(torch.tensor([[v * 0.5, v] for v in self.steps], dtype=torch.float64).reshape(self.K, 2))
        self._init_stream(seed)
        self.n_envs, self.x0_in, self.noise_in, self.u_in = n_envs, x0_in, noise_in, u_in
        self.record = False           # also keep the chain's start points, noise, final samples and energies (last_x0, last_noise, last_x, last_energies)
        self.last_picks = self.last_u = self.last_x0 = self.last_noise = self.last_x = self.last_energies = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, n_envs: int | None = None, device=None, **banks):
        """From a live reference ``IBCAgent`` (duck-typed): ``agent.model.mlp.state_dict()``, ``agent.sampler``'s settings and f64 bounds, ``agent.scaler``; with
        ``agent.use_ema`` the EMA shadow parameters (the reference swaps them in for every predict)."""
        mlp, smp = agent.model.mlp, agent.sampler
        net = ResidualMLP.from_reference_state(mlp.state_dict(), device)
        scaler = Scaler.from_reference(agent.scaler, net.layers[0].weight.device)
        steps = ibc_step_sizes(smp.inference_iterations, smp.sampler_stepsize_init_infer, smp.sampler_stepsize_init, smp.sampler_stepsize_final, smp.sampler_stepsize_power,
                               smp.second_inference_stepsize_init, bool(smp.second_infer))
        pol = cls(net, scaler, steps, noise_scale=smp.noise_scale_infer, delta_action_clip=smp.delta_action_clip, samples=int(smp.inference_samples), seed=seed, n_envs=n_envs,
                  bounds=smp.bounds, **banks)
        if getattr(agent, "use_ema", False):
            pol.use_ema(agent.ema_helper.shadow_params)
        return pol

    @staticmethod
    def matches(agent) -> bool:
        """Is ``agent`` exactly what this policy restates: an IBCAgent without goal conditioning whose sampler is a plain LangevinMCMCSampler (none of its
        subclasses) on the polynomial schedule and whose model is an EBMMLP around a Mish ResidualMLPNetwork without norm and without spectral norm, with one
        output, at most 64 samples and 63 iterations?  Everything else stays on the row-by-row adapter, which runs the reference's own code."""
        try:
            smp, ebm = agent.sampler, agent.model
            if type(smp).__name__ != "LangevinMCMCSampler" or not getattr(smp, "_use_polynomial_rate", False) or not hasattr(smp, "infer_schedule"):
                return False
            if agent.goal_conditioning is not False or type(ebm).__name__ != "EBMMLP" or not hasattr(agent, "scaler") or smp.bounds is None:
                return False
            layers = list(ebm.mlp.layers)
            if not ResidualMLP.is_plain(layers, strict=False) or layers[-1].out_features != 1:
                return False
            K = int(smp.inference_iterations) * (2 if smp.second_infer else 1)
            return int(smp.inference_iterations) >= 2 and K <= 63 and 1 <= int(smp.inference_samples) <= 64 and 1 <= smp.bounds.shape[1] <= 8
        except (AttributeError, TypeError, ValueError, IndexError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy; no per-lane state: the step word is all a capture puts back)
    SWITCH, LAST = "D3IL_POLICY_IBC_FUSED", ("last_picks", "last_u", "last_x0", "last_noise", "last_x", "last_energies")
    TAKES = "the energy network takes %d"

    def load_reference_state_dict(self, sd):
        """``EBMMLP.state_dict()`` of the reference: the network sits under ``mlp.``."""
        self.model.load_state_dict({k[len("mlp."):]: v for k, v in sd.items() if k.startswith("mlp.")})

    # ---- packed tables
    def _pack(self):
        """pack_resmlp_weights of the network; the same packer on the transposed square layers (``wT_blk``) and on the action columns of the input layer as a
        16-row output tile (``wT_act``: row a = W_in[:, obs + a])."""
        from types import SimpleNamespace as NS
        lin_in, blocks, lin_out = self.model._parts()
        out = pack_resmlp_weights(lin_in, blocks, lin_out)
        tr = [tuple(NS(weight=l.weight.t(), bias=l.bias) for l in b) for b in blocks]
        out["wT_blk"] = pack_resmlp_weights(lin_in, tr, lin_out)["w_blk"]
        act = NS(weight=lin_in.weight[:, self.obs_dim:].t(), bias=torch.zeros(self.A, device=lin_in.weight.device), out_features=self.A)
        out["wT_act"] = pack_resmlp_weights(lin_in, [], act)["w_out"]
        return out

    # ---- the chain
    def _kernel_shape(self) -> bool:
        lin_in, blocks, _ = self.model._parts()
        return lin_in.out_features in (128, 256) and len(blocks) <= 4 and lin_in.in_features <= 28 and self.S == 64

    def _banks(self, n, dev, need_host: bool):
        """(x0, noise, u) as the torch path takes them / as the kernel is handed them: the given banks, or (``need_host``) the host form of the kernel's draws."""
        S, A, K, draw = self.S, self.A, self.K, lambda fn, shape, host: self._draw(fn, n, shape, host, need_host, dev)
        x0 = draw(self.x0_in, (n, S, A), lambda t: ibc_start_uniforms(self.seed, self.env_offset, n, t, A, S))
        if x0 is not None and self.x0_in is None:
            x0 = self.lo + x0 * (self.hi - self.lo)
        nz = draw(self.noise_in, (K, n, S, A), lambda t: np.stack([ibc_normals(self.seed, self.env_offset, n, t, k, A, S) for k in range(K)]) if K else np.zeros((0, n, S, A)))
        return x0, nz, draw(self.u_in, (n,), lambda t: ibc_pick_uniforms(self.seed, self.env_offset, n, t))

    def _chain_torch(self, s, x0=None, noise=None, u=None):
        """Steps 1 - 3 of csrc/policy_ibc.h as torch ops in the dtype of ``s`` and the parameters (f32 in the policy; the tests run it in f64 too): returns
        (actions, picks, final samples, energies)."""
        n, S, A, dt = s.shape[0], self.S, self.A, s.dtype
        c = lambda v: v.to(device=s.device, dtype=dt)
        if x0 is None:
            x0, noise, u = self._banks(n, s.device, True)
        d = lambda v: v.to(device=s.device, dtype=torch.float64)
        lo, hi, clip, coef = d(self.lo), d(self.hi), d(self.clip), d(self.coef)
        x = d(x0).reshape(n * S, A)      # the samples are carried in f64 (the reference's f64 bounds promote them), the network runs in ``dt``
        st = s.unsqueeze(1).expand(n, S, s.shape[1]).reshape(n * S, s.shape[1])
        bad = ~torch.isfinite(s).all(dim=1) | ~torch.isfinite(x).reshape(n, -1).all(dim=1)
        for k in range(self.K):
            _, g = resmlp_energy_and_grad(self.model, torch.cat([st, x.to(dt)], dim=1), self.obs_dim)
            raw = coef[k, 0] * g.double() + coef[k, 1] * (d(noise[k]).reshape(n * S, A) * self.noise_scale)
            x = torch.minimum(torch.maximum(x - torch.minimum(torch.maximum(raw, -clip), clip), lo), hi)
            bad |= ~(torch.isfinite(raw) & torch.isfinite(x)).reshape(n, -1).all(dim=1)
        e, _ = resmlp_energy_and_grad(self.model, torch.cat([st, x.to(dt)], dim=1), self.obs_dim, grad=False)
        e, x = e.reshape(n, S), x.reshape(n, S, A)
        bad |= ~torch.isfinite(e).all(dim=1)
        p = torch.exp(-(e - e.min(dim=1, keepdim=True).values))
        cdf = torch.cumsum(p, dim=1)
        picks = (cdf <= c(u).unsqueeze(1) * cdf[:, -1:]).sum(dim=1).clamp_max(S - 1)
        y = self._action_tail(x[torch.arange(n, device=s.device), picks], bad, f64=True, dt=dt)
        return y, torch.where(bad, torch.full_like(picks, -1), picks).to(torch.int32), x.to(dt), e

    def _step_torch(self, s):
        x0, nz, u = self._banks(s.shape[0], s.device, True)
        y, self.last_picks, self.last_x, self.last_energies = self._chain_torch(s, x0, nz, u)
        self.last_u, self.last_x0, self.last_noise = u, x0, nz
        return y

    def _step_kernel(self, s):
        from . import capi
        n, dev, S, A, K = s.shape[0], s.device, self.S, self.A, self.K
        w = self._packed.current(self._pack_params(), self._pack)
        x0, nz, u = self._banks(n, dev, False)
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
        y, picks, u_out = new(n, A), new(n, dtype=torch.int32), new(n)
        xf, en, x0o, nzo = (new(n, S, A), new(n, S), new(n, S, A), new(K, n, S, A)) if self.record else (None, None, None, None)
        lin_in, blocks, _ = self.model._parts()
        capi.launch("d3il_ibc_langevin_f32", dev, state=s, **resmlp_args(w), w_out=w["w_out"], b_out=w["b_out"], wT_blocks=w["wT_blk"], wT_in_act=w["wT_act"], coef=self.coef,
                    noise_scale=self.noise_scale, clip=self.clip, **self._draw_args(), x0_in=x0, noise_in=nz, u_in=u, actions=y, picks=picks, x_final=xf, energies=en,
                    x0_out=x0o, noise_out=nzo, u_out=u_out, n_env=n, obs_dim=self.obs_dim, A=A, hidden=lin_in.out_features, n_blocks=len(blocks), S=S, K=K)
        self.last_picks, self.last_u, self.last_x, self.last_energies, self.last_x0, self.last_noise = picks, u_out, xf, en, x0o, nzo
        return y

    def _fallback_text(self):
        lin_in, blocks, _ = self.model._parts()
        return ("this network (hidden %d, %d blocks, %d inputs, %d samples) is not one the chain kernel is built for; every call runs the torch chain "
                "with its Philox numbers drawn on the host (a device synchronisation per call, no graph capture)" % (lin_in.out_features, len(blocks), lin_in.in_features, self.S))

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, hidden_dim: int = 128, n_blocks: int = 3, action_scale: float = 0.002, policy_seed: int = 0,
               weight_gain: float = 1.0, **kw):
        """A policy of the reference's shape with fixed random weights (there are no checkpoints offline) and the shipped sampler settings of
        configs/agents/ibc_agent.yaml (64 samples, 10 + 10 iterations, step sizes 0.5 / 0.0493 -> 1e-5 with power 2, then 1e-5; noise scale 0.5; clip 0.1): torch's
        default layer initialisation times ``weight_gain``, unit observation scaling, actions of ``action_scale`` per unit of the scaled space, bounds +-1.5."""
        net, sc = ResidualMLP.random(obs_dim + action_dim, hidden_dim, n_blocks, 1, seed, weight_gain), Scaler.unit(obs_dim, action_dim, action_scale, 1.5, device)
        return cls(net.to(device), sc, ibc_step_sizes(10, 0.5, 0.0493, 1e-5, 2.0, 1e-5, True), noise_scale=0.5, delta_action_clip=0.1, seed=policy_seed, **kw)


# ------------------------------------------------------------------------------------------------ VAE-ACT: encoder-decoder transformer that emits action chunks
ACT_TAG = 0x41430000          # fourth Philox counter word of the chunk kernel, or-ed with q < 8 (csrc/policy_act.h; never 0, BET_TAG, a DDPM_GPT_TAG or an IBC_TAG word)


def act_latent_words(seed: int, env_offset: int, n: int, t: int):
    """The Philox words of the chunk kernel: uint32 [n, 8 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t, ACT_TAG | q))."""
    return philox_words(seed, env_offset, n, t, np.uint64(ACT_TAG) | _tag_axes(8)[0])


def act_latent_uniforms(seed: int, env_offset: int, n: int, t: int):
    """The kernel's latent of environments 0 .. n-1 at step word t: float32 [n, 32] in [0, 1 - 2^-24], component 4 q + m = 24 bits of word m of call q
    (the reference draws torch.rand: uniform, not normal)."""
    return uniform24(act_latent_words(seed, env_offset, n, t).reshape(n, 32))


def act_reference_shapes(obs_dim: int, action_dim: int, T: int, C: int = 64, enc_layers: int = 2, dec_layers: int = 4, latent_dim: int = 32, action_enc_layers: int = 2) -> dict:
    """Name -> shape of every parameter of the reference's ActVAE (act_vae.py:325-376; the mask buffers are not parameters and are left out), the training-only
    ones included: what ``act_synthetic_state`` is drawn over, so that the tests rebuild the golden generator's weights without storing them."""
    out = {"state_encoder.weight": (C, obs_dim), "action_embed.weight": (C, action_dim), "latent_out_proj.weight": (C, latent_dim), "action_head.weight": (action_dim, C),
           "action_head.bias": (action_dim,), "latent_proj.weight": (2 * latent_dim, C), "latent_proj.bias": (2 * latent_dim,), "query_embed.weight": (T, C),
           "cls_embed.weight": (1, C), "pos_emb": (1, T, C), "act_pos_emb": (1, T + 1, C)}
    for stack, n, cross in (("encoder", enc_layers, False), ("decoder", dec_layers, True), ("action_encoder", action_enc_layers, False)):
        out[stack + ".ln.weight"] = (C,)
        for i in range(n):
            p = "%s.blocks.%d." % (stack, i)
            out[p + "ln1.weight"] = out[p + "ln2.weight"] = (C,)
            for l in ("key", "query", "value", "proj") + (("cross_key", "cross_query", "cross_value") if cross else ()):
                out[p + "attn.%s.weight" % l], out[p + "attn.%s.bias" % l] = (C, C), (C,)
            out[p + "mlp.0.weight"], out[p + "mlp.0.bias"], out[p + "mlp.2.weight"], out[p + "mlp.2.bias"] = (4 * C, C), (4 * C,), (C, 4 * C), (C,)
    return out


def act_synthetic_state(shapes: dict, seed: int) -> dict:
    """Fixed-seed weights of trained-like magnitudes for an ActVAE-shaped state dict (there are no checkpoints offline; the reference's initialisation, std 0.02
    and zero biases, makes the network nearly linear): one np.random.RandomState(seed), drawn in sorted key order - matrices N(0, 1) 1.2 / sqrt(fan-in) (the action head 2.4: scaled actions of order 2), LayerNorm
    weights 1 + 0.15 N, biases 0.2 N, embeddings and position tables 0.4 N, all rounded to f32.  The golden generator and the tests rebuild the same arrays."""
    rs = np.random.RandomState(seed)
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        z = rs.standard_normal(shape)
        leaf = k.split(".")
        if leaf[-1] == "weight" and leaf[-2] in ("ln", "ln1", "ln2"):
            v = 1.0 + 0.15 * z
        elif leaf[-1] == "bias":
            v = 0.2 * z
        elif leaf[-1] == "weight" and len(shape) == 2 and leaf[-2] not in ("query_embed", "cls_embed"):
            v = z * ((2.4 if leaf[-2] == "action_head" else 1.2) / math.sqrt(shape[1]))
        else:
            v = 0.4 * z
        out[k] = v.astype(np.float32)
    return out


class _ActLayerNorm(nn.Module):      # act_vae.py:26-35 with bias=False
    def __init__(self, ndim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(ndim))

    def forward(self, x):
        return F.layer_norm(x, self.weight.shape, self.weight, None, 1e-5)


class _ActAttention(nn.Module):      # act_vae.py:38-102 (SelfAttention) and 105-167 (CausalSelfCrossAttention), dropout off
    def __init__(self, n_embd, n_heads, block_size, cross):
        super().__init__()
        self.key, self.query, self.value = nn.Linear(n_embd, n_embd), nn.Linear(n_embd, n_embd), nn.Linear(n_embd, n_embd)
        if cross:
            self.cross_key, self.cross_query, self.cross_value = nn.Linear(n_embd, n_embd), nn.Linear(n_embd, n_embd), nn.Linear(n_embd, n_embd)
        self.proj = nn.Linear(n_embd, n_embd)
        self.register_buffer("mask", torch.tril(torch.ones(block_size, block_size)).view(1, 1, block_size, block_size), persistent=False)
        self.n_head = n_heads

    def forward(self, x, cross_input=None):
        B, T, C = x.shape
        hd = C // self.n_head
        sp = lambda v: v.view(B, -1, self.n_head, hd).transpose(1, 2)
        q, k, v = sp(self.query(x)), sp(self.key(x)), sp(self.value(x))
        att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hd))
        att = att.masked_fill(self.mask[:, :, :T, :T] == 0, float("-inf"))      # (a 1 x 1 slice broadcasts: a block_size of 1 masks nothing on two tokens)
        y = F.softmax(att, dim=-1) @ v
        if cross_input is not None:
            kc, vc, qc = sp(self.cross_key(cross_input)), sp(self.cross_value(cross_input)), sp(self.cross_query(x))
            y = y + F.softmax((qc @ kc.transpose(-2, -1)) * (1.0 / math.sqrt(hd)), dim=-1) @ vc
        return self.proj(y.transpose(1, 2).contiguous().view(B, T, C))


class _ActBlock(nn.Module):          # act_vae.py:170-239
    def __init__(self, n_embd, n_heads, block_size, cross):
        super().__init__()
        self.ln1, self.ln2 = _ActLayerNorm(n_embd), _ActLayerNorm(n_embd)
        self.attn = _ActAttention(n_embd, n_heads, block_size, cross)
        self.mlp = nn.Sequential(nn.Linear(n_embd, 4 * n_embd), nn.GELU(), nn.Linear(4 * n_embd, n_embd))

    def forward(self, x, cond=None):
        x = x + self.attn(self.ln1(x), cond)
        return x + self.mlp(self.ln2(x))


class _ActStack(nn.Module):          # act_vae.py:242-305
    def __init__(self, n_embd, n_heads, n_layers, block_size, cross):
        super().__init__()
        self.blocks = nn.Sequential(*[_ActBlock(n_embd, n_heads, block_size, cross) for _ in range(n_layers)])
        self.ln = _ActLayerNorm(n_embd)

    def forward(self, x, cond=None):
        for b in self.blocks:
            x = b(x, cond)
        return self.ln(x)


class ActNet(nn.Module):
    """The inference path of the reference's ActVAE (act_vae.py:389-445 with action = None, goal = None) under the reference's parameter names; the training-only
    parts (action_encoder, action_embed, latent_proj, cls_embed, act_pos_emb) are not held.  ``forward(state [N, obs], latent [N, L]) -> [N, T, A]``; the latent is
    an argument (the reference draws torch.rand inside)."""

    def __init__(self, state_dim, action_dim, act_seq_size, hidden_dim=64, n_heads=4, enc_layers=2, dec_layers=4, latent_dim=32):
        super().__init__()
        self.encoder = _ActStack(hidden_dim, n_heads, enc_layers, act_seq_size, False)
        self.decoder = _ActStack(hidden_dim, n_heads, dec_layers, act_seq_size, True)
        self.state_encoder = nn.Linear(state_dim, hidden_dim, bias=False)
        self.latent_out_proj = nn.Linear(latent_dim, hidden_dim, bias=False)
        self.action_head = nn.Linear(hidden_dim, action_dim)
        self.query_embed = nn.Embedding(act_seq_size, hidden_dim)
        self.pos_emb = nn.Parameter(torch.zeros(1, act_seq_size, hidden_dim))
        self.T, self.A, self.obs_dim, self.C, self.n_head, self.latent_dim = act_seq_size, action_dim, state_dim, hidden_dim, n_heads, latent_dim

    def forward(self, state, latent):
        n = state.shape[0]
        x = torch.stack([self.state_encoder(state), self.latent_out_proj(latent)], dim=1)
        x = x + self.pos_emb[:, :2]      # (T = 1: one row, broadcast onto both tokens)
        enc = self.encoder(x)
        dec = self.decoder(self.query_embed.weight.unsqueeze(0).expand(n, -1, -1), enc)
        return self.action_head(dec)


def pack_tiles(W: torch.Tensor) -> torch.Tensor:
    """A weight matrix [out, in] in the A-operand fragment order of the f32 matrix instruction, rows and columns padded to multiples of 16 with zeros:
    [To][t][lane (g, i)][r] = W[16 To + i][16 t + 4 g + r] (the order of pack_resmlp_weights' square layers)."""
    dev = W.device
    R, Cc = -(-W.shape[0] // 16) * 16, -(-W.shape[1] // 16) * 16
    Wp = torch.zeros(R, Cc, device=dev, dtype=torch.float32)
    Wp[:W.shape[0], :W.shape[1]] = W.detach()
    ar = lambda k: torch.arange(k, device=dev)
    To, t, g, i, r = ar(R // 16)[:, None, None, None, None], ar(Cc // 16)[None, :, None, None, None], ar(4)[None, None, :, None, None], ar(16)[None, None, None, :, None], ar(4)[None, None, None, None, :]
    return Wp[16 * To + i, 16 * t + 4 * g + r].reshape(R // 16, Cc // 16, 64, 4).contiguous()


def pack_act_weights(net: ActNet) -> dict:
    """ActNet in the operand order of csrc/policy_act.h (width 64, latent 32, obs <= 32, T <= 8, A <= 8): every matrix through ``pack_tiles``;
    w_in = [state_encoder (columns padded to 32) | latent_out_proj]; per encoder layer enc_w = [query key value proj fc1 fc2], enc_v = [ln1 ln2 b_query b_key b_value
    b_proj b_fc1 b_fc2]; per decoder layer dec_w = [query key value cross_query cross_key cross_value proj fc1 fc2], dec_v alike; head_w = action_head (rows padded to
    16); tab = [pos (2 rows: pos_emb[0, :2], for T = 1 row 0 twice) | query_embed (padded to 8 rows) | encoder.ln | decoder.ln | head bias (padded to 16)]."""
    assert net.C == 64 and net.latent_dim == 32 and net.obs_dim <= 32 and net.T <= 8 and net.A <= 8
    flat = lambda *xs: torch.cat([x.detach().to(torch.float32).reshape(-1) for x in xs])
    dev = net.pos_emb.device
    se = torch.zeros(64, 32, device=dev)
    se[:, :net.obs_dim] = net.state_encoder.weight.detach()
    pos = net.pos_emb.detach()[0, :2].expand(2, 64)
    qe = torch.zeros(8, 64, device=dev)
    qe[:net.T] = net.query_embed.weight.detach()
    hb = torch.zeros(16, device=dev)
    hb[:net.A] = net.action_head.bias.detach()
    enc_w, enc_v, dec_w, dec_v = [], [], [], []
    for b in net.encoder.blocks:
        a = b.attn
        enc_w.append(flat(*[pack_tiles(l.weight) for l in (a.query, a.key, a.value, a.proj, b.mlp[0], b.mlp[2])]))
        enc_v.append(flat(b.ln1.weight, b.ln2.weight, a.query.bias, a.key.bias, a.value.bias, a.proj.bias, b.mlp[0].bias, b.mlp[2].bias))
    for b in net.decoder.blocks:
        a = b.attn
        dec_w.append(flat(*[pack_tiles(l.weight) for l in (a.query, a.key, a.value, a.cross_query, a.cross_key, a.cross_value, a.proj, b.mlp[0], b.mlp[2])]))
        dec_v.append(flat(b.ln1.weight, b.ln2.weight, a.query.bias, a.key.bias, a.value.bias, a.cross_query.bias, a.cross_key.bias, a.cross_value.bias, a.proj.bias, b.mlp[0].bias, b.mlp[2].bias))
    return {"w_in": flat(pack_tiles(se), pack_tiles(net.latent_out_proj.weight)), "tab": flat(pos, qe, net.encoder.ln.weight, net.decoder.ln.weight, hb),
            "enc_w": torch.stack(enc_w), "enc_v": torch.stack(enc_v), "dec_w": torch.stack(dec_w), "dec_v": torch.stack(dec_v), "head_w": flat(pack_tiles(net.action_head.weight))}


class ACTPolicy(_ChunkLanes, NativePolicy):
    """ActAgent.predict without goals (agents/act_agent.py:207-239) around ActVAE.forward without actions (act_vae.py:389-445), on a batch: scale the observation;
    a lane whose ``counter`` equals the chunk length T is due and computes a new chunk of T actions from its CURRENT observation and a fresh uniform latent -
    clamped to the scaler's bounds in the scaled space, inverse-scaled, stored -; every lane then emits chunk[counter] and counts on.  ``reset()`` makes all lanes
    due, ``begin_episodes(mask)`` the masked ones (an environment that restarts mid-chunk falls out of phase with its neighbours: the state is per lane).

    On a HIP device the whole call is ONE kernel (csrc/policy_act.h through d3il_act_chunk_f32: width 64, 4 heads, latent 32, obs <= 32, A <= 8, T <= 8, at most
    4 encoder and 8 decoder layers), then a device-side add on the step word; a call in which no lane of a 16-lane tile is due costs that tile only the emit.  On the
    CPU, for other shapes and with D3IL_POLICY_ACT_FUSED=0 the same arithmetic runs as torch ops (``_chunk_torch``) on the same Philox stream computed on the
    host - that path cannot be captured.  Random numbers: Philox4x32-10 keyed by ``seed`` with counter (env_offset + lane, step word, ACT_TAG | q);
    ``latent_in(n) -> [n, 32]`` replaces the draw when given (golden replay, tests).  A NaN / Inf in a due lane's state row or head outputs gives that lane a NaN
    chunk."""

    def __init__(self, model: ActNet, scaler: Scaler, seed: int = 0, n_envs: int | None = None, latent_in=None):
        self.model, self.scaler = model.eval(), scaler
        dev = scaler.x_mean.device
        self.device = dev
        self.T, self.A, self.obs_dim = int(model.T), int(model.A), int(model.obs_dim)
        assert scaler.y_bounds is not None and tuple(scaler.y_bounds.shape) == (2, self.A), "ACTPolicy clamps to the scaler's y_bounds"
        self._init_output(scaler)
        self._init_stream(seed)
        self.n_envs, self.latent_in = n_envs, latent_in
        self.counter = self.chunk = self.last_latent = None          # per-lane state: i32 [N], f32 [N, T, A] (clamped, inverse-scaled), the latent of the lane's chunk [N, 32]
        self.record = False           # also keep a copy of the chunk table after every call (last_chunk)
        self.last_chunk = None
        if n_envs is not None:
            self._state(int(n_envs))

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, n_envs: int | None = None, device=None, latent_in=None):
        """From a live reference ``ActAgent`` (duck-typed): ``agent.model.state_dict()`` (the training-only keys are ignored) and ``agent.scaler``."""
        sd = {k: torch.as_tensor(v) for k, v in agent.model.state_dict().items()}
        dev = torch.device(device) if device is not None else sd["state_encoder.weight"].device
        C, obs = sd["state_encoder.weight"].shape
        layers = lambda p: len({k.split(".")[2] for k in sd if k.startswith(p + ".blocks.")})
        net = ActNet(obs, sd["action_head.weight"].shape[0], sd["query_embed.weight"].shape[0], hidden_dim=C, n_heads=int(agent.model.encoder.blocks[0].attn.n_head),
                     enc_layers=layers("encoder"), dec_layers=layers("decoder"), latent_dim=sd["latent_out_proj.weight"].shape[1])
        pol = cls(net.to(dev), Scaler.from_reference(agent.scaler, dev), seed=seed, n_envs=n_envs, latent_in=latent_in)
        pol.load_reference_state_dict(sd)
        return pol

    @staticmethod
    def matches(agent) -> bool:
        """Is ``agent`` exactly what this policy restates: an ActAgent without goal conditioning, obs_size 1, window_size == action_seq_size, whose model is an
        ActVAE without goal encoder whose encoder, decoder, cross and hidden widths are one, LayerNorms without bias?  Everything else stays on the row-by-row
        adapter, which runs the reference's own code."""
        try:
            m = agent.model
            gc = agent.gc if hasattr(agent, "gc") else agent.goal_conditioned
            if gc is not False or int(agent.obs_size) != 1 or int(agent.window_size) != int(agent.action_seq_size) or hasattr(m, "goal_encoder"):
                return False
            if not hasattr(agent, "scaler") or agent.scaler.y_bounds is None or not hasattr(agent, "predict") or not hasattr(agent, "action_counter"):
                return False
            C, T = int(m.state_encoder.out_features), int(agent.action_seq_size)
            if m.state_encoder.bias is not None or m.latent_out_proj.bias is not None or int(m.latent_out_proj.out_features) != C:
                return False
            if tuple(m.query_embed.weight.shape) != (T, C) or tuple(m.pos_emb.shape) != (1, T, C) or int(m.action_head.in_features) != C:
                return False
            heads = set()
            for stack, cross in ((m.encoder, False), (m.decoder, True)):
                if tuple(stack.ln.weight.shape) != (C,) or getattr(stack.ln, "bias", None) is not None or len(stack.blocks) < 1:
                    return False
                for b in stack.blocks:
                    a = b.attn
                    lins = [a.key, a.query, a.value, a.proj] + ([a.cross_key, a.cross_query, a.cross_value] if cross else [])
                    if hasattr(a, "cross_key") != cross or not all(isinstance(l, nn.Linear) and l.in_features == C and l.out_features == C and l.bias is not None for l in lins):
                        return False
                    if any(getattr(ln, "bias", None) is not None or tuple(ln.weight.shape) != (C,) for ln in (b.ln1, b.ln2)):
                        return False
                    if not (isinstance(b.mlp[0], nn.Linear) and isinstance(b.mlp[1], nn.GELU) and getattr(b.mlp[1], "approximate", "none") == "none" and isinstance(b.mlp[2], nn.Linear)):
                        return False
                    if (b.mlp[0].in_features, b.mlp[0].out_features, b.mlp[2].in_features, b.mlp[2].out_features) != (C, 4 * C, 4 * C, C):
                        return False
                    if tuple(a.mask.shape) != (1, 1, T, T):
                        return False
                    heads.add(int(a.n_head))
            return len(heads) == 1 and C % heads.pop() == 0
        except (AttributeError, TypeError, ValueError, IndexError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy)
    SWITCH, STATE, LAST = "D3IL_POLICY_ACT_FUSED", ("counter", "chunk", "last_latent"), ("last_chunk",)
    TAKES = "the state encoder takes %d"

    def _state(self, n):
        """counter / chunk / last_latent for n lanes; a new size starts with every lane due."""
        if self.counter is None or self.counter.shape[0] != n:
            self._chunk_state(n, self.T)
            self.last_latent = torch.zeros(n, self.model.latent_dim, dtype=torch.float32, device=self.device)

    def load_reference_state_dict(self, sd):
        """``ActVAE.state_dict()`` of the reference: a plain load of the keys the inference path has (masks and the training-only modules are ignored)."""
        own = self.model.state_dict()
        self.model.load_state_dict({k: torch.as_tensor(sd[k]).to(own[k].dtype) for k in own})
        for p in self.model.parameters():
            p.requires_grad_(False)

    def _pack(self):
        return pack_act_weights(self.model)

    # ---- the step
    def _kernel_shape(self) -> bool:
        m = self.model
        return (m.C == 64 and m.n_head == 4 and m.latent_dim == 32 and m.obs_dim <= 32 and 1 <= m.A <= 8 and 1 <= m.T <= 8 and 1 <= len(m.encoder.blocks) <= 4
                and 1 <= len(m.decoder.blocks) <= 8)

    def _latent(self, n, dev, need_host: bool):
        return self._draw(self.latent_in, n, (n, self.model.latent_dim), lambda t: act_latent_uniforms(self.seed, self.env_offset, n, t), need_host, dev)

    def _chunk_torch(self, s, z):
        """A new chunk for every row, in the dtype of ``s`` and the parameters (f32 in the policy; the tests run it in f64 too): network, clamp to the bounds in the
        scaled space, inverse scaling as two operations; rows with a NaN / Inf in the state or a head output are NaN."""
        a_hat = self.model(s, z.to(device=s.device, dtype=s.dtype))
        bad = ~torch.isfinite(s).all(dim=1) | ~torch.isfinite(a_hat).reshape(s.shape[0], -1).all(dim=1)
        return self._action_tail(a_hat, bad, False, self.lo, self.hi)

    def _step_torch(self, s):
        if s.is_cuda and _capturing():
            raise RuntimeError("ACTPolicy: the torch path decides on the host which lanes are due and draws its Philox numbers there; it cannot be captured - the kernel can")
        n = s.shape[0]
        due = self._due()
        if bool(due.any()):
            z = self._latent(n, s.device, True)
            new = self._chunk_torch(torch.where(due.unsqueeze(1), s, torch.zeros_like(s)), z)
            self.chunk.copy_(torch.where(due.reshape(-1, 1, 1), new, self.chunk))
            self.last_latent.copy_(torch.where(due.unsqueeze(1), z, self.last_latent))
            self.counter.masked_fill_(due, 0)
        return self._emit()

    def _step_kernel(self, s):
        from . import capi
        n, dev, m = s.shape[0], s.device, self.model
        w = self._packed.current(self._pack_params(), self._pack)
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        capi.launch("d3il_act_chunk_f32", dev, state=s, **w, **self._draw_args(), latent_in=self._latent(n, dev, False), counter=self.counter, chunk=self.chunk, actions=y,
                    latent_out=self.last_latent, n_env=n, obs_dim=self.obs_dim, A=self.A, T=self.T, width=m.C, n_head=m.n_head, latent=m.latent_dim, n_enc=len(m.encoder.blocks),
                    n_dec=len(m.decoder.blocks))
        return y

    def _fallback_text(self):
        return ("this network (width %d, %d heads, latent %d, T %d) is not one the chunk kernel is built for; every call runs the torch path "
                "with a device synchronisation per call and no graph capture" % (self.model.C, self.model.n_head, self.model.latent_dim, self.T))

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, act_seq_size: int = 3, device="cuda", seed: int = 0, enc_layers: int = 2, dec_layers: int = 4, hidden_dim: int = 64,
               n_heads: int = 4, latent_dim: int = 32, action_scale: float = 0.002, bound: float = 1.5, policy_seed: int = 0, **kw):
        """A policy of the reference's shape (configs/agents/act_agent.yaml: 2 encoder and 4 decoder layers, width 64, 4 heads, latent 32) with the fixed
        trained-like weights of ``act_synthetic_state`` (there are no checkpoints offline), unit observation scaling, actions of ``action_scale`` per unit of the
        scaled space, bounds +-``bound``."""
        net = ActNet(obs_dim, action_dim, act_seq_size, hidden_dim, n_heads, enc_layers, dec_layers, latent_dim)
        net.load_state_dict({k: torch.as_tensor(v) for k, v in act_synthetic_state({k: v.shape for k, v in net.state_dict().items()}, seed).items()})
        return cls(net.requires_grad_(False).to(device), Scaler.unit(obs_dim, action_dim, action_scale, bound, device), seed=policy_seed, **kw)


# ------------------------------------------------------------------------------------------------ conditional VAE: a clamped prior sample through the decoder
CVAE_TAG = 0x43560000         # fourth Philox counter word of the decode kernel, or-ed with q < 8 (csrc/policy_cvae.h; never 0, BET_TAG, a DDPM_GPT_TAG, IBC_TAG or ACT_TAG word)
CVAE_Z_BOUND = 0.5            # VariationalAE.predict clamps its prior sample to +-0.5 (cvae.py:58)


def cvae_words(seed: int, env_offset: int, n: int, t: int):
    """The Philox words of the decode kernel: uint32 [n, 8 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t, CVAE_TAG | q))."""
    return philox_words(seed, env_offset, n, t, np.uint64(CVAE_TAG) | _tag_axes(8)[0])


def cvae_latent_normals(seed: int, env_offset: int, n: int, t: int, L: int):
    """The kernel's UNCLAMPED standard normals of environments 0 .. n-1 at step word t: float64 [n, L], component a = 4 q + m from word m of call q.  Exact on the
    words and f64 from there on (``box_muller_f64``: words 0, 1 -> components 0, 1; words 2, 3 -> components 2, 3)."""
    assert 1 <= L <= 32, "the counter layout holds eight calls of four components"
    return box_muller_f64(cvae_words(seed, env_offset, n, t)).reshape(n, 32)[:, :L]


class CVAEPolicy(NativePolicy):
    """CVAEAgent.predict (agents/cvae_agent.py:155-170) around VariationalAE.predict (agents/models/vae/cvae.py:55-62) on a batch: scale the observation, draw a
    standard-normal latent per environment and CLAMP IT TO +-0.5 - the reference clamps its prior sample, so 2 (1 - Phi(0.5)) = 61.7 % of all latent components sit
    exactly on a bound; kept as it is -, run the decoder (a Mish ResidualMLPNetwork) on [state | z] (state first), clamp to the data bounds (scaled space),
    inverse-scale.  The reference's clamp bounds and output scaler are float64: the clamp of the f32 output against them equals the clamp against their f32
    roundings, and the inverse scaling is an f64 product and sum, here on the f32 scale and shift and rounded to f32 once.  The encoder is not part of inference
    and is neither held nor loaded.  No history: the reference runs this agent with window_size 1.

    On a HIP device the whole call is ONE kernel (csrc/policy_cvae.h through d3il_cvae_decode_f32: hidden 128 / 256, latent <= 32, obs + latent <= 64, at most 16
    action components, any number of blocks), then a device-side add on the step word.  On the CPU, for other shapes and with D3IL_POLICY_CVAE_FUSED=0 the same
    arithmetic runs as torch ops (``_decode_torch``) on the same Philox stream computed on the host - that path cannot be captured.  Random numbers: Philox4x32-10
    keyed by ``seed`` with counter (env_offset + lane, step word, CVAE_TAG | q), so results do not depend on batch order, sub-batches or ranks;
    ``z_in(n) -> [n, L]`` (UNCLAMPED normals; the policy clamps them) replaces the draw when given (golden replay, tests); ``last_z`` is the clamped latent that
    was used.  A NaN / Inf in an environment's scaled state row, unclamped latent or decoder output gives that environment NaN in every action component."""

    def __init__(self, decoder: ResidualMLP, scaler: Scaler, latent_dim: int, seed: int = 0, n_envs: int | None = None, z_in=None):
        self.model, self.scaler = decoder.eval(), scaler
        dev = scaler.x_mean.device
        self.device = dev
        lin_in, _, lin_out = decoder._parts()
        self.L, self.A = int(latent_dim), int(lin_out.out_features)
        self.obs_dim = int(lin_in.in_features) - self.L
        assert 1 <= self.L <= 32, "the Philox counter layout holds a latent of at most 32 components"
        assert self.obs_dim >= 1, "the decoder reads [state | latent]"
        self._init_output(scaler)
        self._init_stream(seed)
        self.n_envs, self.z_in = n_envs, z_in
        self.last_z = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, n_envs: int | None = None, device=None, z_in=None):
        """From a live reference ``CVAEAgent`` (duck-typed): ``agent.model.decoder.state_dict()``, ``agent.model.latent_dim``, ``agent.scaler`` (its ``y_bounds`` are
        the clamp).  The encoder is left where it is."""
        net = ResidualMLP.from_reference_state(agent.model.decoder.state_dict(), device)
        return cls(net, Scaler.from_reference(agent.scaler, net.layers[0].weight.device), int(agent.model.latent_dim), seed=seed, n_envs=n_envs, z_in=z_in)

    @staticmethod
    def matches(agent) -> bool:
        """Is ``agent`` exactly what this policy restates: a CVAEAgent whose model is a VariationalAE with a decoder made of plain ``nn.Linear`` layers and Mish
        blocks without norm and without spectral norm, a latent of 1 .. 32 components, at most 64 decoder inputs and 16 outputs?  Everything else stays on the
        row-by-row adapter, which runs the reference's own code."""
        try:
            vae = agent.model
            if type(agent).__name__ != "CVAEAgent" or type(vae).__name__ != "VariationalAE" or not hasattr(agent, "scaler") or agent.scaler.y_bounds is None:
                return False
            layers = list(vae.decoder.layers)
            if not ResidualMLP.is_plain(layers, strict=True):
                return False
            L = int(vae.latent_dim)
            return 1 <= L <= 32 and L < layers[0].in_features <= 64 and 1 <= layers[-1].out_features <= 16
        except (AttributeError, TypeError, ValueError, IndexError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy; no per-lane state: the step word is all a capture puts back)
    SWITCH, LAST, TAKES = "D3IL_POLICY_CVAE_FUSED", ("last_z",), "the decoder takes %d next to its latent"

    def load_reference_state_dict(self, sd):
        """``VariationalAE.state_dict()`` of the reference: the decoder sits under ``decoder.``; the encoder's entries are ignored."""
        self.model.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")})

    def _pack(self):
        """pack_resmlp_weights of the decoder with the input layer packed to 64 columns."""
        return pack_resmlp_weights(*self.model._parts(), in_cols=64)

    # ---- the decode
    def _kernel_shape(self) -> bool:
        lin_in, _, lin_out = self.model._parts()
        return lin_in.out_features in (128, 256) and lin_in.in_features <= 64 and self.L <= 32 and lin_out.out_features <= 16

    def _bank(self, n, dev, need_host: bool):
        """The unclamped latent (``_draw``)."""
        return self._draw(self.z_in, n, (n, self.L), lambda t: cvae_latent_normals(self.seed, self.env_offset, n, t, self.L), need_host, dev)

    def _decode_torch(self, s, z):
        """Steps 1 - 3 of csrc/policy_cvae.h as torch ops in the dtype of ``s`` and the parameters (f32 in the policy; the tests run it in f64 too) on the unclamped
        latent ``z``: returns (actions, the clamped latent)."""
        dt = s.dtype
        z = z.to(device=s.device, dtype=dt)
        zc = z.clamp(-CVAE_Z_BOUND, CVAE_Z_BOUND)
        x = torch.cat([s, zc], dim=1)
        for layer in self.model.layers:
            x = layer(x)
        bad = ~(torch.isfinite(s).all(dim=1) & torch.isfinite(z).all(dim=1) & torch.isfinite(x).all(dim=1))
        return self._action_tail(x, bad, True, self.lo, self.hi), torch.where(torch.isfinite(z), zc, torch.full_like(zc, float("nan")))

    def _step_torch(self, s):
        y, self.last_z = self._decode_torch(s, self._bank(s.shape[0], s.device, True))
        return y

    def _step_kernel(self, s):
        from . import capi
        n, dev = s.shape[0], s.device
        w = self._packed.current(self._pack_params(), self._pack)
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        self.last_z = torch.empty(n, self.L, dtype=torch.float32, device=dev)
        lin_in, blocks, _ = self.model._parts()
        capi.launch("d3il_cvae_decode_f32", dev, state=s, **resmlp_args(w), w_out=w["w_out"], b_out=w["b_out"], **self._draw_args(), z_in=self._bank(n, dev, False), actions=y,
                    z_out=self.last_z, n_env=n, obs_dim=self.obs_dim, latent=self.L, A=self.A, hidden=lin_in.out_features, n_blocks=len(blocks))
        return y

    def _fallback_text(self):
        lin_in = self.model._parts()[0]
        return ("this decoder (hidden %d, %d inputs, %d outputs) is not one the decode kernel is built for; every call runs torch's layers "
                "with the Philox numbers drawn on the host (a device synchronisation per call, no graph capture)" % (lin_in.out_features, lin_in.in_features, self.A))

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, hidden_dim: int = 128, n_blocks: int = 3, latent_dim: int = 16, action_scale: float = 0.002,
               policy_seed: int = 0, weight_gain: float = 1.0, bound: float = 1.5, **kw):
        """A policy of the reference's shape with fixed random weights (there are no checkpoints offline): the shipped scripts use hidden 128 / 256 with 6 / 8 hidden
        layers (3 / 4 blocks) and a latent of 16, 24 or 32; torch's default layer initialisation times ``weight_gain``, unit observation scaling, actions of
        ``action_scale`` per unit of the scaled space, bounds +-``bound``."""
        net, sc = ResidualMLP.random(obs_dim + latent_dim, hidden_dim, n_blocks, action_dim, seed, weight_gain), Scaler.unit(obs_dim, action_dim, action_scale, bound, device)
        return cls(net.to(device), sc, latent_dim, seed=policy_seed, **kw)


# ------------------------------------------------------------------------------------------------ BeT-MLP: the Behaviour Transformer's sampling tail on a residual MLP
BET_MLP_TAG = 0x424D4C50      # fourth Philox counter word of the BeT-MLP kernel (csrc/policy_bet_mlp.h; never 0, never a word of the six tags above)
BET_MLP_EDGE = 1e-4           # a draw this close to an edge of the normalised CDF is not decided between two arithmetics (tests, golden generator)


def bet_mlp_words(seed: int, env_offset: int, n: int, t: int):
    """The Philox words of the BeT-MLP kernel: uint32 [n, 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t, BET_MLP_TAG))."""
    return philox_words(seed, env_offset, n, t, BET_MLP_TAG)


def bet_mlp_uniforms(seed: int, env_offset: int, n: int, t: int):
    """The kernel's uniforms of rows 0 .. n-1 at step word t, on the host: the upper 24 bits of word 0, float32 in [0, 1 - 2^-24]."""
    return uniform24(bet_mlp_words(seed, env_offset, n, t)[:, 0])


def pack_bet_mlp_weights(lin_in, blocks, lin_out, V: int = 64) -> dict:
    """The ResidualMLPNetwork of a BeT-MLP policy for k_bet_mlp: input layer and blocks as ``pack_resmlp_weights`` packs them (32 input columns); rows 0 .. V-1 of the
    output layer (the logits) as V / 16 output tiles in the operand order of its ``w_out`` tile, w_logit [V / 16][NT][lane (g, i)][r] = W[16 T + i][16 t + 4 g + r],
    with b_logit [V]; rows V .. (the offsets, layout "(V A)") row-major as they are, w_off [V A][H] with b_off [V A]."""
    from types import SimpleNamespace
    dev, H = lin_in.weight.device, lin_in.out_features
    NT = H // 16
    assert V % 16 == 0 and lin_out.out_features % V == 0 and lin_out.out_features > V and lin_out.in_features == H and lin_out.bias is not None
    none = SimpleNamespace(out_features=0, weight=torch.zeros(0, H, device=dev), bias=torch.zeros(0, device=dev))
    pk = pack_resmlp_weights(lin_in, blocks, none)
    del pk["w_out"], pk["b_out"]
    ar = lambda k: torch.arange(k, device=dev)
    T, t, g, i, r = ar(V // 16)[:, None, None, None, None], ar(NT)[None, :, None, None, None], ar(4)[None, None, :, None, None], ar(16)[None, None, None, :, None], ar(4)[None, None, None, None, :]
    f = lambda x: x.detach().to(torch.float32).contiguous()
    W, b = lin_out.weight, lin_out.bias
    pk.update(w_logit=f(W[16 * T + i, 16 * t + 4 * g + r].reshape(V // 16, NT, 64, 4)), b_logit=f(b[:V]), w_off=f(W[V:]), b_off=f(b[V:]))
    return pk


class BeTMLPPolicy(NativePolicy):
    """BetMLP_Agent.predict (agents/bet_mlp_agent.py:366-406) on a batch: scale the observation (no history - the agent's ``obs_context`` is never read in predict,
    the reference feeds a [1, 1, obs] row), run the Mish ResidualMLPNetwork whose output layer (WITH bias) has V (1 + A) rows, softmax over the first V, ONE
    categorical draw, the offsets of the drawn bin in the layout "(V A)" (generate_latents, same file 114-147), bin_centers[bin] + offset in f32
    (k_means.py decode_actions), clamp to the data bounds IN SCALED SPACE (the f32 sum against the f64 bounds: the same as against their f32 roundings), inverse
    scaling as an f64 product and sum on the f32 scale and shift, rounded to f32 once (the reference's output scaler is f64) - the dtypes CVAEPolicy has.

    The draw is BeTPolicy's: bin = min(#{v : c_v <= u S}, V - 1), c the inclusive prefix sums of exp(logit - max), S = c_{V-1}, on ONE uniform per lane and step -
    24 bits of Philox4x32-10 keyed by ``seed`` with counter (env_offset + lane, step word, BET_MLP_TAG), independent of batch order, sub-batches and ranks, unlike
    torch.multinomial's device generator - or ``uniform_fn(n) -> [n]`` when given (golden replay, tests).

    On a HIP device the whole call is ONE kernel (csrc/policy_bet_mlp.h through d3il_bet_mlp_f32: hidden 128 / 256, V = 64, obs <= 28, A <= 8, any number of blocks),
    then a device-side add on the step word, so a captured graph draws fresh numbers at every replay.  On the CPU, for other shapes and with
    D3IL_POLICY_BET_MLP_FUSED=0 the same arithmetic runs as torch ops (``_predict_torch``) with the uniforms computed on the host - that path cannot be captured.
    An environment with a NaN / Inf in its scaled state row, final hidden row or logits gets bin -1 and NaN in every action component."""

    def __init__(self, model: ResidualMLP, bin_centers, scaler: Scaler, seed: int = 0, uniform_fn=None):
        self.model, self.scaler = model.eval(), scaler
        dev = scaler.x_mean.device
        self.device = dev
        f = lambda a: torch.as_tensor(a).detach().to(device=dev, dtype=torch.float32).contiguous()
        self.centers = f(bin_centers)
        self.V, self.A = int(self.centers.shape[0]), int(self.centers.shape[1])
        lin_in, _, lin_out = model._parts()
        self.obs_dim = int(lin_in.in_features)
        assert lin_out.out_features == self.V * (1 + self.A) and lin_out.bias is not None, "the output layer has V (1 + A) rows and a bias"
        self._init_output(scaler)
        self._init_stream(seed)
        self.uniform_fn = uniform_fn
        self.record = False           # also keep the probabilities (last_probs)
        self.last_bins = self.last_u = self.last_probs = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, uniform_fn=None, device=None):
        """From a live reference ``BetMLP_Agent`` (duck-typed): ``agent.model.model.state_dict()`` (the ResidualMLPNetwork), ``agent.action_ae.bin_centers``,
        ``agent.scaler`` (its ``y_bounds`` are the clamp)."""
        net = ResidualMLP.from_reference_state(agent.model.model.state_dict(), device)
        scaler = Scaler.from_reference(agent.scaler, net.layers[0].weight.device)
        return cls(net, torch.as_tensor(agent.action_ae.bin_centers), scaler, seed=seed, uniform_fn=uniform_fn)

    @staticmethod
    def matches(agent) -> bool:
        """Is ``agent`` exactly what this policy restates: a BetMLP_Agent whose policy predicts offsets on 64 bins with a ResidualMLPNetwork of plain ``nn.Linear``
        layers and Mish blocks without norm and without spectral norm, an ``nn.Identity`` observation encoder, bin centres [64, A] with A <= 8 and a scaler with
        bounds?  Everything else stays on the row-by-row adapter, which runs the reference's own code."""
        try:
            pol = agent.model
            if type(agent).__name__ != "BetMLP_Agent" or not hasattr(agent, "scaler") or agent.scaler.y_bounds is None:
                return False
            if not pol.predict_offsets or int(pol.vocab_size) != 64 or type(agent.obs_encoding_net) is not nn.Identity:
                return False
            layers = list(pol.model.layers)
            if not ResidualMLP.is_plain(layers, strict=True):
                return False
            centers = torch.as_tensor(agent.action_ae.bin_centers)
            if centers.dim() != 2 or centers.shape[0] != 64 or not 1 <= centers.shape[1] <= 8:
                return False
            return layers[-1].out_features == 64 * (1 + centers.shape[1]) and int(getattr(pol, "act_dim", centers.shape[1])) == centers.shape[1]
        except (AttributeError, TypeError, ValueError, IndexError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy; no per-lane state: the step word is all a capture puts back)
    SWITCH, LAST = "D3IL_POLICY_BET_MLP_FUSED", ("last_bins", "last_u", "last_probs")

    def load_reference_state_dict(self, sd):
        """``ResidualMLPNetwork.state_dict()`` of the reference (bet_mlp_agent.py: agent.model.model)."""
        self.model.load_state_dict(sd)

    def _pack(self):
        return pack_bet_mlp_weights(*self.model._parts(), V=self.V)

    def _kernel_shape(self) -> bool:
        lin_in, _, _ = self.model._parts()
        return lin_in.out_features in (128, 256) and 1 <= lin_in.in_features <= 28 and self.V == 64 and 1 <= self.A <= 8

    # ---- the call
    def _uniforms(self, n, dev, need_host: bool):
        return self._draw(self.uniform_fn, n, (n,), lambda t: bet_mlp_uniforms(self.seed, self.env_offset, n, t), need_host, dev)

    def _tail_torch(self, s, h, out, u):
        """Steps 3 - 7 of csrc/policy_bet_mlp.h as torch ops in the dtype of ``out`` (f32 in the policy; the tests run it in f64 too), in the kernel's order of
        operations where the order is defined (S is the last prefix sum): returns (actions, bins i32, probabilities)."""
        V, A, dt, dev = self.V, self.A, out.dtype, out.device
        logits = out[:, :V]
        p = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        c = torch.cumsum(p, dim=1)
        S = c[:, -1:]
        bins = (c <= u.to(dev, dt).unsqueeze(1) * S).sum(dim=1).clamp_max(V - 1)
        off = out[:, V:].reshape(-1, V, A)[torch.arange(out.shape[0], device=dev), bins]
        bad = ~(torch.isfinite(s).all(dim=1) & torch.isfinite(h).all(dim=1) & torch.isfinite(logits).all(dim=1))
        y = self._action_tail(self.centers.to(dev, dt)[bins] + off, bad, True, self.lo, self.hi)
        return y, torch.where(bad, torch.full_like(bins, -1), bins).to(torch.int32), p / S

    def _predict_torch(self, s, u):
        """Steps 1 - 7 on torch's layers: (actions, bins, probabilities)."""
        h = s
        for layer in self.model.layers[:-1]:
            h = layer(h)
        return self._tail_torch(s, h, self.model.layers[-1](h), u)

    def _step_torch(self, s):
        u = self._uniforms(s.shape[0], s.device, True)
        y, self.last_bins, probs = self._predict_torch(s, u)
        self.last_u, self.last_probs = u, probs if self.record else None
        return y

    def _step_kernel(self, s):
        from . import capi
        n, dev = s.shape[0], s.device
        w = self._packed.current(self._pack_params(), self._pack)
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        bins = torch.empty(n, dtype=torch.int32, device=dev)
        u_out = torch.empty(n, dtype=torch.float32, device=dev)
        probs = torch.empty(n, self.V, dtype=torch.float32, device=dev) if self.record else None
        lin_in, blocks, _ = self.model._parts()
        capi.launch("d3il_bet_mlp_f32", dev, state=s, **resmlp_args(w), w_logit=w["w_logit"], b_logit=w["b_logit"], w_off=w["w_off"], b_off=w["b_off"], centers=self.centers,
                    **self._draw_args(), u_in=self._uniforms(n, dev, False), actions=y, bins=bins, u_out=u_out, probs=probs, n_env=n, obs_dim=self.obs_dim, V=self.V, A=self.A,
                    hidden=lin_in.out_features, n_blocks=len(blocks))
        self.last_bins, self.last_u, self.last_probs = bins, u_out, probs
        return y

    def _fallback_text(self):
        return ("this network (hidden %d, %d inputs, %d bins, %d action components) is not one the kernel is built for; every call runs "
                "torch's layers with the Philox numbers drawn on the host (a device synchronisation per call, no graph capture)"
                % (self.model._parts()[0].out_features, self.obs_dim, self.V, self.A))

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, hidden_dim: int = 128, n_blocks: int = 3, action_scale: float = 0.002, policy_seed: int = 0,
               logit_std: float = 2.0, bound: float = 1.5, uniform_fn=None):
        """A policy of the reference's shape with fixed random weights (there are no checkpoints offline): the shipped scripts use hidden 128 / 256 with 6 / 8 hidden
        layers (3 / 4 blocks) and 64 bins; torch's default layer initialisation, the logit rows scaled to logits of a standard deviation of about ``logit_std`` (neither
        uniform nor one-hot), small offsets, centres of 0.9, unit observation scaling, actions of ``action_scale`` per unit of the scaled space, bounds +-``bound``."""
        g = torch.Generator().manual_seed(seed)
        net = ResidualMLP.random(obs_dim, hidden_dim, n_blocks, 64 * (1 + action_dim), seed)
        with torch.no_grad():
            out = net.layers[-1]
            out.weight[:64] = torch.randn(64, hidden_dim, generator=g) * (logit_std / hidden_dim ** 0.5)
            out.weight[64:] = torch.randn(64 * action_dim, hidden_dim, generator=g) * (0.4 / hidden_dim ** 0.5)
            out.bias.copy_(torch.randn(out.bias.shape, generator=g) * 0.1)
        sc = Scaler.unit(obs_dim, action_dim, action_scale, bound, device)
        return cls(net.to(device), torch.randn(64, action_dim, generator=g) * 0.9, sc, seed=policy_seed, uniform_fn=uniform_fn)


# ------------------------------------------------------------------------------------------------ BC-GMM: a Gaussian mixture head on a residual MLP, sampled once per step
BC_GMM_TAG = 0x474D0000       # fourth Philox counter word of the BC-GMM kernel, or-ed with q: 0 the uniform, 1 / 2 the normals (csrc/policy_bc_gmm.h; its upper half is no other tag's)
BC_GMM_EDGE = 1e-4            # a draw this close to an edge of the normalised CDF is not decided between two arithmetics (tests, golden generator)
BC_GMM_LOW_NOISE_STD = 1e-4   # robomimic's low_noise_eval, which bc_gmm.py:74-75 takes over
BC_GMM_STD_MODES = {"low_noise": 0, "exp": 1, "softplus": 2}      # std_mode of d3il_bc_gmm


def bc_gmm_words(seed: int, env_offset: int, n: int, t: int):
    """The Philox words of the BC-GMM kernel: uint32 [n, 3 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t, BC_GMM_TAG | q))."""
    return philox_words(seed, env_offset, n, t, np.uint64(BC_GMM_TAG) | _tag_axes(3)[0])


def bc_gmm_uniforms(seed: int, env_offset: int, n: int, t: int):
    """The kernel's uniforms of rows 0 .. n-1 at step word t, on the host: the upper 24 bits of word 0 of call q = 0, float32 in [0, 1 - 2^-24]."""
    return uniform24(bc_gmm_words(seed, env_offset, n, t)[:, 0, 0])


def bc_gmm_normals(seed: int, env_offset: int, n: int, t: int, A: int):
    """The kernel's standard normals of rows 0 .. n-1 at step word t: float64 [n, A], component a = 4 (q - 1) + m from word m of call q = 1, 2.  Exact on the words
    and f64 from there on (``box_muller_f64``: words 0, 1 -> components 0, 1; words 2, 3 -> components 2, 3), as ``cvae_latent_normals``."""
    assert 1 <= A <= 8, "the counter layout holds two calls of four components"
    return box_muller_f64(bc_gmm_words(seed, env_offset, n, t)[:, 1:3]).reshape(n, 8)[:, :A]


class GMMNet(nn.Module):
    """BC_GMM (agents/models/gmm/bc_gmm.py:13-90) without its distribution objects: ``mlp`` a Mish ResidualMLPNetwork whose output layer has ``hidden_dim`` rows
    (mlp_output_dim = hidden_dim, as every shipped config sets it), and the three heads ``mean_mlp`` / ``std_mlp`` [G A rows, layout "(G A)"] and ``logits_mlp``
    [G rows] under the reference's parameter names."""

    def __init__(self, input_dim, hidden_dim, num_hidden_layers, output_dim, n_gaussians):
        super().__init__()
        self.mlp = ResidualMLP(input_dim, hidden_dim, num_hidden_layers, hidden_dim)
        self.mean_mlp, self.std_mlp = nn.Linear(hidden_dim, output_dim * n_gaussians), nn.Linear(hidden_dim, output_dim * n_gaussians)
        self.logits_mlp = nn.Linear(hidden_dim, n_gaussians)
        self.n_gaussians, self.output_dim = int(n_gaussians), int(output_dim)

    @classmethod
    def from_reference_state(cls, sd, device=None):
        """The network of a reference ``BC_GMM.state_dict()`` - widths, block count, G and A read from the shapes -, loaded, on ``device`` (default: where the state
        dict lives), frozen."""
        sd = {k: torch.as_tensor(v) for k, v in sd.items()}
        hidden, in_dim = sd["mlp.layers.0.weight"].shape
        G = sd["logits_mlp.weight"].shape[0]
        rows = sd["mean_mlp.weight"].shape[0]
        assert rows % G == 0 and sd["std_mlp.weight"].shape[0] == rows, "mean_mlp and std_mlp have n_gaussians * output_dim rows"
        net = cls(in_dim, hidden, 2 * len({k.split(".")[2] for k in sd if ".l1." in k}), rows // G, G)
        net.load_state_dict(sd)
        return net.to(torch.device(device) if device is not None else sd["mlp.layers.0.weight"].device).requires_grad_(False).eval()


def pack_bc_gmm_weights(net: GMMNet) -> dict:
    """A GMMNet for k_bc_gmm: input layer and blocks as ``pack_resmlp_weights`` packs them (32 input columns); the trunk's output layer as one more square layer,
    w_feat [T_out][t][lane (g, i)][r] = W_o[16 T_out + i][16 t + 4 g + r] with b_feat [H]; the G logit rows padded to 64 with zeros, as four output tiles in the same
    operand order, w_logit [4][NT][64][4] with b_logit [64]; the mean and std rows (layout "(G A)") row-major as they are, w_mean / w_std [G A][H] with b_mean / b_std."""
    from types import SimpleNamespace
    lin_in, blocks, lin_out = net.mlp._parts()
    dev, H, G = lin_in.weight.device, lin_in.out_features, net.n_gaussians
    NT = H // 16
    assert lin_out.out_features == H and lin_out.in_features == H and 1 <= G <= 64 and net.logits_mlp.out_features == G
    none = SimpleNamespace(out_features=0, weight=torch.zeros(0, H, device=dev), bias=torch.zeros(0, device=dev))
    pk = pack_resmlp_weights(lin_in, blocks, none)
    del pk["w_out"], pk["b_out"]
    ar = lambda k: torch.arange(k, device=dev)
    t, g, i, r = ar(NT)[None, :, None, None, None], ar(4)[None, None, :, None, None], ar(16)[None, None, None, :, None], ar(4)[None, None, None, None, :]
    tiles = lambda W, n: W[16 * ar(n)[:, None, None, None, None] + i, 16 * t + 4 * g + r].reshape(n, NT, 64, 4)
    f = lambda x: x.detach().to(torch.float32).contiguous()
    wl, bl = torch.zeros(64, H, device=dev), torch.zeros(64, device=dev)
    wl[:G], bl[:G] = net.logits_mlp.weight, net.logits_mlp.bias
    pk.update(w_feat=f(tiles(lin_out.weight, NT)), b_feat=f(lin_out.bias), w_logit=f(tiles(wl, 4)), b_logit=f(bl), w_mean=f(net.mean_mlp.weight), b_mean=f(net.mean_mlp.bias),
              w_std=f(net.std_mlp.weight), b_std=f(net.std_mlp.bias))
    return pk


class BCGMMPolicy(NativePolicy):
    """The BC-GMM agent on a batch.  The reference ships the model (agents/models/gmm/bc_gmm.py), its config (configs/agents/bc_gmm_agent.yaml) and its benchmark
    scripts, but no agents/bc_gmm_agent.py; the yaml has BC_Agent's constructor keys, so the contract restated here is BC_Agent.predict (agents/bc_agent.py:240-271)
    with ``model(state).sample()`` in place of ``model(state)``: window 1, no history, one sample per step as robomimic's GMMActorNetwork does.  Per environment:
    scale the observation, h = input layer and blocks of the Mish ResidualMLPNetwork, f = Mish(output layer(h)) (no activation in front of that layer; it has
    hidden_dim rows), logits = logits_mlp(f), ONE categorical draw k, mean = 0.01 tanh(mean_mlp(f))[k], std = 1e-4 with ``low_noise_eval`` (the shipped default;
    std_mlp is not evaluated) or act(std_mlp(f))[k] + min_std with act = exp or torch's softplus, x = mean + std z, clamp to the data bounds IN SCALED SPACE,
    inverse scaling as an f64 product and sum on the f32 scale and shift, rounded to f32 once - the dtypes CVAEPolicy and BeTMLPPolicy have.
    ``use_tanh_wrapped_distribution`` is not restated: such a model stays on the row-by-row adapter.

    MixtureSameFamily.sample draws a [1, 1, G, A] block of normals and keeps the drawn component's A values; this policy draws only the A normals it uses - the
    same distribution with fewer draws.  The component is BeTMLPPolicy's inverse CDF: k = min(#{g : c_g <= u S}, G - 1) on the inclusive prefix sums of
    exp(logit - max), on ONE uniform per lane and step; the normals are Box-Muller pairs.  Both come from Philox4x32-10 keyed by ``seed`` with counter (env_offset +
    lane, step word, BC_GMM_TAG | q) - q = 0 the uniform, q = 1, 2 four normals each -, independent of batch order, sub-batches and ranks; ``u_in(n) -> [n]`` and
    ``z_in(n) -> [n, A]`` replace them when given (golden replay, tests).  ``last_comps``, ``last_u``, ``last_z`` (and ``last_probs`` with ``record``) are what was used.

    On a HIP device the whole call is ONE kernel (csrc/policy_bc_gmm.h through d3il_bc_gmm: hidden 128 / 256, obs <= 28, G <= 64, A <= 8, any number of blocks), then
    a device-side add on the step word, so a captured graph draws fresh numbers at every replay.  On the CPU, for other shapes and with D3IL_POLICY_BC_GMM_FUSED=0 the
    same arithmetic runs as torch ops (``_predict_torch``) with the numbers drawn on the host - that path cannot be captured.  An environment with a NaN / Inf in
    its scaled state row, in f, in a logit, in its selected raw mean or std, in its std or in a normal it uses gets component -1 and NaN in every action component."""

    def __init__(self, model: GMMNet, scaler: Scaler, min_std: float = 1e-4, std_activation: str = "exp", low_noise_eval: bool = True, seed: int = 0, u_in=None, z_in=None):
        assert std_activation in ("exp", "softplus"), "std_activation is exp or softplus"
        self.model, self.scaler = model.eval(), scaler
        self.device = scaler.x_mean.device
        lin_in, _, lin_out = model.mlp._parts()
        self.G, self.A, self.obs_dim = int(model.n_gaussians), int(model.output_dim), int(lin_in.in_features)
        assert lin_out.out_features == lin_in.out_features, "mlp_output_dim equals hidden_dim"
        assert 1 <= self.G <= 64 and 1 <= self.A <= 8, "the Philox counter layout and the draw hold 64 mixture components of 8 action components"
        self.min_std, self.std_activation, self.low_noise_eval = float(min_std), std_activation, bool(low_noise_eval)
        self._init_output(scaler)
        self._init_stream(seed)
        self.u_in, self.z_in = u_in, z_in
        self.record = False           # also keep the probabilities (last_probs)
        self.last_comps = self.last_u = self.last_z = self.last_probs = None

    @property
    def std_mode(self) -> int:
        return BC_GMM_STD_MODES["low_noise" if self.low_noise_eval else self.std_activation]

    # ---- construction from the reference's objects
    @classmethod
    def from_model(cls, state_dict, scaler, min_std: float = 1e-4, std_activation: str = "exp", low_noise_eval: bool = True, seed: int = 0, device=None, u_in=None, z_in=None):
        """From a reference ``BC_GMM.state_dict()`` (a checkpoint) and a scaler with the reference's attributes; the model's three settings as the config states them."""
        net = GMMNet.from_reference_state(state_dict, device)
        return cls(net, Scaler.from_reference(scaler, net.logits_mlp.weight.device), min_std, std_activation, low_noise_eval, seed=seed, u_in=u_in, z_in=z_in)

    @classmethod
    def from_reference(cls, agent, seed: int = 0, device=None, u_in=None, z_in=None):
        """From a live ``BC_GMM_Agent`` (duck-typed, BC_Agent's attributes): ``agent.model`` (a BC_GMM: state dict, min_std, std_activation, low_noise_eval),
        ``agent.scaler`` (its ``y_bounds`` are the clamp)."""
        m = agent.model
        return cls.from_model(m.state_dict(), agent.scaler, float(m.min_std), str(m.std_activation), bool(m.low_noise_eval), seed=seed, device=device, u_in=u_in, z_in=z_in)

    @staticmethod
    def matches(agent) -> bool:
        """Is ``agent`` exactly what this policy restates: a BC_GMM_Agent whose model is a BC_GMM in eval mode (in train mode low_noise_eval is ignored) with a
        ResidualMLPNetwork of plain ``nn.Linear`` layers and Mish blocks without norm and without spectral norm, mlp_output_dim = hidden_dim, Mish behind it, three
        plain ``nn.Linear`` heads of G A, G A and G rows, no tanh-wrapped distribution, std_activation exp or softplus, 1 <= G <= 64, 1 <= A <= 8 and a scaler with
        bounds?  Everything else stays on the row-by-row adapter, which runs the reference's own code."""
        try:
            m = agent.model
            if type(agent).__name__ != "BC_GMM_Agent" or type(m).__name__ != "BC_GMM" or not hasattr(agent, "scaler") or agent.scaler.y_bounds is None:
                return False
            if m.training or m.use_tanh_wrapped_distribution or m.std_activation not in ("exp", "softplus") or not isinstance(m.mlp_output_act, nn.Mish):
                return False
            layers = list(m.mlp.layers)
            if not ResidualMLP.is_plain(layers, strict=True) or layers[-1].out_features != layers[0].out_features:
                return False
            G, A, H = int(m.n_gaussians), int(m.output_dim), layers[0].out_features
            heads = ((m.mean_mlp, G * A), (m.std_mlp, G * A), (m.logits_mlp, G))
            if not all(type(l) is nn.Linear and not hasattr(l, "weight_orig") and l.bias is not None and l.in_features == H and l.out_features == rows for l, rows in heads):
                return False
            return 1 <= G <= 64 and 1 <= A <= 8
        except (AttributeError, TypeError, ValueError, IndexError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy; no per-lane state: the step word is all a capture puts back)
    SWITCH, LAST = "D3IL_POLICY_BC_GMM_FUSED", ("last_comps", "last_u", "last_z", "last_probs")

    def load_reference_state_dict(self, sd):
        """``BC_GMM.state_dict()`` of the reference."""
        self.model.load_state_dict(sd)

    def _pack(self):
        return pack_bc_gmm_weights(self.model)

    def _kernel_shape(self) -> bool:
        lin_in = self.model.mlp._parts()[0]
        return lin_in.out_features in (128, 256) and 1 <= lin_in.in_features <= 28 and 1 <= self.G <= 64 and 1 <= self.A <= 8

    # ---- the call
    def _uniforms(self, n, dev, need_host: bool):
        return self._draw(self.u_in, n, (n,), lambda t: bc_gmm_uniforms(self.seed, self.env_offset, n, t), need_host, dev)

    def _normals(self, n, dev, need_host: bool):
        return self._draw(self.z_in, n, (n, self.A), lambda t: bc_gmm_normals(self.seed, self.env_offset, n, t, self.A), need_host, dev)

    def _predict_torch(self, s, u, z):
        """Steps 1 - 8 of csrc/policy_bc_gmm.h as torch ops in the dtype of ``s`` and the parameters (f32 in the policy; the tests run it in f64 too), in the
        kernel's order of operations where the order is defined (S is the last prefix sum; the product std z is rounded before the sum): returns (actions,
        components i32, probabilities)."""
        m, G, A, dt, dev = self.model, self.G, self.A, s.dtype, s.device
        h = s
        for layer in m.mlp.layers[:-1]:
            h = layer(h)
        f = F.mish(m.mlp.layers[-1](h))
        logits = m.logits_mlp(f)
        p = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        c = torch.cumsum(p, dim=1)
        S = c[:, -1:]
        k = (c <= u.to(dev, dt).unsqueeze(1) * S).sum(dim=1).clamp_max(G - 1)
        ar = torch.arange(s.shape[0], device=dev)
        mraw = m.mean_mlp(f).reshape(-1, G, A)[ar, k]
        mean = 0.01 * torch.tanh(mraw)
        if self.low_noise_eval:
            sraw, sd = torch.zeros_like(mraw), torch.full_like(mraw, BC_GMM_LOW_NOISE_STD)
        else:
            sraw = m.std_mlp(f).reshape(-1, G, A)[ar, k]
            sd = (torch.exp(sraw) if self.std_activation == "exp" else F.softplus(sraw)) + self.min_std
        z = z.to(dev, dt)
        x = mean + sd * z
        fin = lambda v: torch.isfinite(v).all(dim=1)
        bad = ~(fin(s) & fin(f) & fin(logits) & fin(mraw) & fin(sraw) & fin(sd) & fin(z))
        y = self._action_tail(x, bad, True, self.lo, self.hi)
        return y, torch.where(bad, torch.full_like(k, -1), k).to(torch.int32), p / S

    def _step_torch(self, s):
        n = s.shape[0]
        if self.u_in is None or self.z_in is None:
            self._host_step_word()      # (raises under a capture before anything is drawn)
        u, z = self._uniforms(n, s.device, True), self._normals(n, s.device, True)
        y, self.last_comps, probs = self._predict_torch(s, u, z)
        self.last_u, self.last_z, self.last_probs = u, z, probs if self.record else None
        return y

    def _step_kernel(self, s):
        from . import capi
        n, dev = s.shape[0], s.device
        w = self._packed.current(self._pack_params(), self._pack)
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        comps = torch.empty(n, dtype=torch.int32, device=dev)
        u_out = torch.empty(n, dtype=torch.float32, device=dev)
        z_out = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        probs = torch.empty(n, self.G, dtype=torch.float32, device=dev) if self.record else None
        lin_in, blocks, _ = self.model.mlp._parts()
        low = self.low_noise_eval
        d = self._draw_args()
        capi.launch("d3il_bc_gmm", dev, n_env=n, t_device=d["t_device"], state=s, **resmlp_args(w), w_feat=w["w_feat"], b_feat=w["b_feat"], w_logit=w["w_logit"], b_logit=w["b_logit"],
                    w_mean=w["w_mean"], b_mean=w["b_mean"], w_std=None if low else w["w_std"], b_std=None if low else w["b_std"], lo=d["lo"], hi=d["hi"], scale=d["scale"],
                    shift=d["shift"], seed=self.seed, env_offset=self.env_offset, u_in=self._uniforms(n, dev, False), z_in=self._normals(n, dev, False), actions=y, comps=comps,
                    u_out=u_out, z_out=z_out, probs=probs, obs_dim=self.obs_dim, G=self.G, A=self.A, hidden=lin_in.out_features, n_blocks=len(blocks), std_mode=self.std_mode,
                    min_std=self.min_std)
        self.last_comps, self.last_u, self.last_z, self.last_probs = comps, u_out, z_out, probs
        return y

    def _fallback_text(self):
        return ("this network (hidden %d, %d inputs, %d mixture components, %d action components) is not one the kernel is built for; every call runs "
                "torch's layers with the Philox numbers drawn on the host (a device synchronisation per call, no graph capture)"
                % (self.model.mlp._parts()[0].out_features, self.obs_dim, self.G, self.A))

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, hidden_dim: int = 128, n_blocks: int = 3, n_gaussians: int = 8, action_scale: float = 0.5,
               policy_seed: int = 0, logit_std: float = 2.0, bound: float = 1.5, min_std: float = 1e-4, std_activation: str = "exp", low_noise_eval: bool = True, u_in=None,
               z_in=None):
        """A policy of the reference's shape with fixed random weights (there are no checkpoints offline): the shipped scripts use hidden 128 / 256 with 6 / 8 hidden
        layers (3 / 4 blocks) and 8 .. 64 components; torch's default layer initialisation, the logit rows scaled so that the logits of standard-normal inputs have a
        standard deviation of about ``logit_std`` (neither uniform nor one-hot), mean rows that use the range of the tanh, std rows around exp(-1), unit observation
        scaling, actions of ``action_scale`` per unit of the scaled space (the means are at most 0.01 there), bounds +-``bound``."""
        g = torch.Generator().manual_seed(seed)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            net = GMMNet(obs_dim, hidden_dim, 2 * n_blocks, action_dim, n_gaussians)
        net.requires_grad_(False).eval()
        with torch.no_grad():
            x = torch.randn(256, obs_dim, generator=g)
            for layer in net.mlp.layers:
                x = layer(x)
            rms = float(F.mish(x).pow(2).mean().sqrt())
            net.logits_mlp.weight.copy_(torch.randn(n_gaussians, hidden_dim, generator=g) * (logit_std / (rms * hidden_dim ** 0.5)))
            net.mean_mlp.weight.copy_(torch.randn(n_gaussians * action_dim, hidden_dim, generator=g) * (1.0 / (rms * hidden_dim ** 0.5)))
            net.std_mlp.weight.copy_(torch.randn(n_gaussians * action_dim, hidden_dim, generator=g) * (0.5 / (rms * hidden_dim ** 0.5)))
            net.std_mlp.bias.copy_(torch.randn(n_gaussians * action_dim, generator=g) * 0.1 - 1.0)
        sc = Scaler.unit(obs_dim, action_dim, action_scale, bound, device)
        return cls(net.to(device), sc, min_std, std_activation, low_noise_eval, seed=policy_seed, u_in=u_in, z_in=z_in)


# ------------------------------------------------------------------------------------------------ BC-GPT: the minGPT trunk with a regression head
class GPTBCPolicy(BeTPolicy):
    """Gpt_Agent.predict (agents/gpt_bc_agent.py:221-247) on a batch: scaled observation window (deque maxlen W; the window GROWS at episode start), the minGPT
    trunk - the BeT library's GPT with vocab_size = action_dim (agents/models/transformer/gpt_policy.py), so ``ln_f`` and a BIAS-FREE head of A rows - and at every
    lane's last token the tail: ln_f, the head, clamp to the data bounds IN SCALED SPACE (the f32 output against the f64 bounds: the same as against their f32
    roundings), inverse scaling as an f64 product and sum on the f32 scale and shift, rounded to f32 once (the reference's output scaler is f64).  No random numbers;
    the step word is advanced all the same (the protocol of NativePolicy).

    The window handling is BeTPolicy's, inherited: ``_History``, the lockstep and the right-padded path, ``begin_episodes``, the fixed-shape chain of a capture and the
    blocks' packed weights.  On a HIP device the tail is one kernel (csrc/policy_gpt_bc.h through d3il_gpt_bc_head_f32; C <= 128, A <= 16); on the CPU, for other
    shapes and with D3IL_POLICY_GPT_BC_HEAD=0 the same arithmetic as torch ops (``_tail_torch``).  A lane with a NaN / Inf in its hidden row, its normalised row or
    a head output gets NaN in every action component (``last_bad``)."""

    SWITCH, LAST = "D3IL_POLICY_GPT_BC_HEAD", ("last_bad",)

    def __init__(self, trunk: MinGPTTrunk, scaler: Scaler, window_size: int, seed: int = 0):
        self.trunk, self.scaler, self.W = trunk.eval(), scaler, int(window_size)
        dev = scaler.x_mean.device
        self.device = dev
        self.A = int(trunk.head.weight.shape[0])
        assert trunk.head.bias is None and trunk.block_size >= self.W
        self._init_output(scaler)
        assert self.min_action.numel() == self.A, "one bound per head row"
        self._init_stream(seed)
        self.hist = None
        self._static = False          # fixed-shape chain with device-only state (set by capture_snapshot)
        self.last_bad = None

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, device=None):
        """From a live reference ``Gpt_Agent`` (duck-typed): ``agent.model.model.model.state_dict()`` (the GPT), ``agent.scaler`` (its ``y_bounds`` are the clamp),
        ``agent.window_size``."""
        mingpt = agent.model.model
        sd = mingpt.model.state_dict()
        dev = torch.device(device) if device is not None else sd["tok_emb.weight"].device
        n_embd, input_dim = sd["tok_emb.weight"].shape
        n_layer = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        n_head = int(getattr(mingpt, "n_head", 0) or mingpt.model.blocks[0].attn.n_head)
        trunk = MinGPTTrunk(input_dim, n_embd, n_layer, n_head, sd["pos_emb"].shape[1], sd["head.weight"].shape[0], 0)
        trunk.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        return cls(trunk.to(dev).requires_grad_(False), Scaler.from_reference(agent.scaler, dev), int(agent.window_size), seed=seed)

    @staticmethod
    def matches(agent) -> bool:
        """Is ``agent`` exactly what this policy restates: a Gpt_Agent around GptPolicy / MinGPT with continuous input, an ``nn.Identity`` observation encoder, no
        visual input, a bias-free head of one row per action component and a scaler with bounds?  Everything else stays on the row-by-row adapter."""
        try:
            pol = agent.model
            if type(agent).__name__ != "Gpt_Agent" or not hasattr(agent, "scaler") or agent.scaler.y_bounds is None or getattr(pol, "visual_input", False):
                return False
            if type(pol.obs_encoder) is not nn.Identity:
                return False
            gpt = pol.model.model
            sd = gpt.state_dict()
            if "head.bias" in sd or "tok_emb.bias" not in sd or sd["tok_emb.weight"].dim() != 2 or "ln_f.weight" not in sd:
                return False
            A = sd["head.weight"].shape[0]
            W = int(agent.window_size)
            return 1 <= A == int(np.asarray(agent.scaler.y_bounds).shape[1]) and 1 <= W <= sd["pos_emb"].shape[1] and sd["head.weight"].shape[1] == sd["tok_emb.weight"].shape[0]
        except (AttributeError, TypeError, ValueError, IndexError, KeyError):
            return False

    # ---- the tail
    def head_kernel_ok(self, h) -> bool:
        C = h.shape[-1]
        return h.is_cuda and h.dtype == torch.float32 and C <= 128 and C % 4 == 0 and 1 <= self.A <= 16 and self.trunk.head.weight.dtype == torch.float32 and self._switch_on()

    def _tail_torch(self, h):
        """Steps 1 - 3 of csrc/policy_gpt_bc.h as torch ops in the dtype of ``h`` and the parameters (f32 in the policy; the tests run it in f64 too)."""
        x = self.trunk.ln_f(h)
        o = F.linear(x, self.trunk.head.weight)
        bad = ~(torch.isfinite(h).all(dim=1) & torch.isfinite(x).all(dim=1) & torch.isfinite(o).all(dim=1))
        self.last_bad = bad.to(torch.int32)
        return self._action_tail(o, bad, True, self.min_action, self.max_action)

    def _tail_kernel(self, h):
        from . import capi
        n, C = h.shape
        h = h.contiguous()
        dev = h.device
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        bad = torch.empty(n, dtype=torch.int32, device=dev)
        ln, w = self.trunk.ln_f, self.trunk.head.weight
        assert w.is_contiguous()
        capi.launch("d3il_gpt_bc_head_f32", dev, h=h, ln_weight=ln.weight, ln_bias=ln.bias, ln_eps=float(ln.eps), w_head=w, lo=self.min_action, hi=self.max_action,
                    scale=self.out_scale, shift=self.out_shift, actions=y, bad=bad, rows=n, C=C, A=self.A)
        self.last_bad = bad
        return y

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, n_embd: int = 120, n_layer: int = 6, n_head: int = 6, window_size: int = 5,
               action_scale: float = 0.002, policy_seed: int = 0, head_gain: float = 1.0, bound: float = 1.5):
        """A BC-GPT policy of the reference's shape (n_embd 72 or 120, window 1 or 5) with fixed random weights - there are no checkpoints offline: torch's default
        layer initialisation, head rows that give outputs of about ``head_gain`` in the scaled space, unit observation scaling, actions of ``action_scale`` per unit
        of the scaled space, bounds +-``bound``."""
        g = torch.Generator().manual_seed(seed)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            trunk = MinGPTTrunk(obs_dim, n_embd, n_layer, n_head, window_size, action_dim, 0)
        with torch.no_grad():
            trunk.pos_emb.copy_(torch.randn(trunk.pos_emb.shape, generator=g) * 0.1)
            trunk.head.weight.copy_(torch.randn(action_dim, n_embd, generator=g) * (head_gain / n_embd ** 0.5))
        return cls(trunk.requires_grad_(False).to(device), Scaler.unit(obs_dim, action_dim, action_scale, bound, device), window_size, seed=policy_seed)


# ------------------------------------------------------------------------------------------------ DDPM-ACT: encoder-decoder diffusion sampler that emits action chunks
DDPM_ACT_TAG = 0x44410000     # fourth Philox counter word of the chain kernel, or-ed with k << 8 | j << 1 | q (csrc/policy_ddpm_act.h; never 0, never a word of the five tags above)


def ddpm_act_words(seed: int, env_offset: int, n: int, t: int, k: int, Ta: int):
    """The Philox words behind ``ddpm_act_normals``: uint32 [n, Ta, 2 (q), 4] = Philox4x32-10(key = seed, counter = (lo32, hi32 of env_offset + row, t,
    DDPM_ACT_TAG | k << 8 | j << 1 | q)), j the action token."""
    assert 1 <= k <= 255 and 1 <= Ta <= 4, "the counter layout holds k <= 255; chain index 0 is never drawn; chunks of at most 4"
    j, q = _tag_axes(Ta, 2)
    return philox_words(seed, env_offset, n, t, np.uint64(DDPM_ACT_TAG | (k << 8)) | (j << np.uint64(1)) | q)


def ddpm_act_normals(seed: int, env_offset: int, n: int, t: int, k: int, Ta: int, A: int):
    """The chain kernel's normals of environments 0 .. n-1 at step word t and chain index k (T = the first iterate, i = reverse step i), on the host: float64
    [n, Ta, A].  Exact on the 32-bit words and f64 from there on (``box_muller_f64``); component a = 4 q + m."""
    assert 1 <= A <= 8
    return box_muller_f64(ddpm_act_words(seed, env_offset, n, t, k, Ta)).reshape(n, Ta, 8)[:, :, :A]


def ddpm_act_reference_shapes(obs_dim: int, action_dim: int, obs_seq_len: int, action_seq_len: int, C: int = 64, enc_layers: int = 2, dec_layers: int = 4) -> dict:
    """Name -> shape of every parameter of the reference's DiffusionEncDec with a linear head (diffusion_models.py:687-765; the mask buffers are not parameters), in
    the reference's ``named_parameters()`` order: what ``ddpm_act_synthetic_state`` is drawn over."""
    out = {"pos_emb": (1, obs_seq_len - 1 + action_seq_len, C)}
    for stack, n, cross in (("encoder", enc_layers, False), ("decoder", dec_layers, True)):
        for i in range(n):
            p = "%s.blocks.%d." % (stack, i)
            out[p + "ln1.weight"] = out[p + "ln2.weight"] = (C,)
            for l in ("key", "query", "value") + (("cross_key", "cross_query", "cross_value") if cross else ()) + ("proj",):
                out[p + "attn.%s.weight" % l], out[p + "attn.%s.bias" % l] = (C, C), (C,)
            out[p + "mlp.0.weight"], out[p + "mlp.0.bias"], out[p + "mlp.2.weight"], out[p + "mlp.2.bias"] = (4 * C, C), (4 * C,), (C, 4 * C), (C,)
        out[stack + ".ln.weight"] = (C,)
    out.update({"tok_emb.weight": (C, obs_dim), "tok_emb.bias": (C,), "time_emb.1.weight": (2 * C, C), "time_emb.1.bias": (2 * C,), "time_emb.3.weight": (C, 2 * C),
                "time_emb.3.bias": (C,), "action_emb.weight": (C, action_dim), "action_emb.bias": (C,), "action_pred.weight": (action_dim, C), "action_pred.bias": (action_dim,)})
    return out


DDPM_ACT_HEAD_ALIGN = 3.0


def ddpm_act_synthetic_state(shapes: dict, seed: int) -> dict:
    """Fixed-seed weights of trained-like magnitudes for a DiffusionEncDec-shaped state dict (there are no checkpoints offline; the reference's initialisation, std
    0.02 and zero biases, makes the network nearly linear): the rule of ``act_synthetic_state`` - one np.random.RandomState(seed), drawn in sorted key order,
    matrices N(0, 1) 1.2 / sqrt(fan-in), LayerNorm weights 1 + 0.15 N, biases 0.2 N, the position table 0.4 N, all rounded to f32.  One trait of a trained
    denoiser is added afterwards: row a of the noise head ``action_pred`` gets DDPM_ACT_HEAD_ALIGN times the direction in which ``action_emb`` writes component a
    into the residual stream (column a over its squared norm), so that the noise estimate follows the iterate.  A head that ignores the iterate makes
    x0 = sqrt(1 / ac) x - sqrt(1 / ac - 1) eps grow from step to step and EVERY chain ends on the clamp bounds; with it some final entries sit on a bound and most
    do not."""
    rs = np.random.RandomState(seed)
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        z = rs.standard_normal(shape)
        leaf = k.split(".")
        if leaf[-1] == "weight" and leaf[-2] in ("ln", "ln1", "ln2"):
            v = 1.0 + 0.15 * z
        elif leaf[-1] == "bias":
            v = 0.2 * z
        elif leaf[-1] == "weight" and len(shape) == 2:
            v = z * (1.2 / math.sqrt(shape[1]))
        else:
            v = 0.4 * z
        out[k] = v.astype(np.float32)
    if "action_pred.weight" in out and "action_emb.weight" in out:      # the trained trait: the noise estimate follows the iterate
        e = out["action_emb.weight"].astype(np.float64)
        out["action_pred.weight"] = (out["action_pred.weight"] + DDPM_ACT_HEAD_ALIGN * (e / (e * e).sum(axis=0, keepdims=True)).T).astype(np.float32)
    return out


class EncDecDenoiser(nn.Module):
    """The inference path of the reference's DiffusionEncDec (diffusion_models.py:687-905), not goal conditioned, under the reference's parameter names - ``pos_emb``,
    ``encoder.*``, ``decoder.*``, ``tok_emb``, ``time_emb.1 / .3``, ``action_emb``, ``action_pred``, registered in the reference's order - so the entries of
    ``Diffusion.state_dict()`` under ``model.`` load with ``load_state_dict`` and EMA shadow lists zip onto ``parameters()``.  Encoder input [time token, state
    tokens + pos[0:L]] through ``_ActStack`` with its causal mask; the action tokens add pos[L-1 : L-1+Ta] - the offset follows the window length L -; the decoder
    attends causally over the action tokens and unmasked over all 1 + L encoder rows."""

    def __init__(self, state_dim, action_dim, embed_dim=64, n_heads=4, enc_layers=2, dec_layers=4, obs_seq_len=5, action_seq_len=4, block_size=9, linear_output=True):
        super().__init__()
        assert block_size >= 1 + obs_seq_len and block_size >= action_seq_len, "the causal masks are block_size wide: they must cover 1 + obs_seq_len encoder tokens"
        self.encoder = _ActStack(embed_dim, n_heads, enc_layers, block_size, False)
        self.decoder = _ActStack(embed_dim, n_heads, dec_layers, block_size, True)
        self.tok_emb = nn.Linear(state_dim, embed_dim)
        self.pos_emb = nn.Parameter(torch.zeros(1, obs_seq_len - 1 + action_seq_len, embed_dim))
        self.time_emb = nn.Sequential(_SinusoidalPosEmb(embed_dim), nn.Linear(embed_dim, embed_dim * 2), nn.Mish(), nn.Linear(embed_dim * 2, embed_dim))
        self.action_emb = nn.Linear(action_dim, embed_dim)
        self.action_pred = nn.Linear(embed_dim, action_dim) if linear_output else nn.Sequential(nn.Linear(embed_dim, 100), nn.GELU(), nn.Linear(100, action_dim))
        self.goal_conditioned = False
        self.state_dim, self.action_dim, self.embed_dim, self.n_heads, self.linear_output = state_dim, action_dim, embed_dim, n_heads, bool(linear_output)
        self.obs_seq_len, self.action_seq_len, self.block_size = obs_seq_len, action_seq_len, block_size

    def time_tokens(self, time):
        """time_emb of integer chain steps [b] -> [b, C], the sinusoid's frequencies in the parameters' dtype (the reference builds them in the default dtype)."""
        dt, half = self.tok_emb.weight.dtype, self.embed_dim // 2
        freq = torch.exp(torch.arange(half, device=time.device).to(dt) * -(math.log(10000) / (half - 1)))
        emb = time.reshape(-1).to(dt)[:, None] * freq[None, :]
        x = torch.cat((emb.sin(), emb.cos()), dim=-1)
        for layer in list(self.time_emb)[1:]:
            x = layer(x)
        return x

    def encode(self, time, states):
        """The encoder output [b, 1 + L, C] of chain step ``time`` [b] on the window ``states`` [b, L, obs]: it does not depend on the iterate."""
        L = states.shape[1]
        return self.encoder(torch.cat([self.time_tokens(time).unsqueeze(1), self.tok_emb(states) + self.pos_emb[:, :L]], dim=1))

    def decode(self, actions, enc):
        L = enc.shape[1] - 1
        Ta = actions.shape[1]
        return self.action_pred(self.decoder(self.action_emb(actions) + self.pos_emb[:, L - 1:L - 1 + Ta], enc))

    def forward(self, actions, time, states, goals=None):
        """The reference's forward without goals: eps [b, Ta, A] for actions [b, Ta, A], time [b] (integers) and states [b, L, state_dim], 1 <= L <= obs_seq_len."""
        assert actions.shape[1] == self.action_seq_len and 1 <= states.shape[1] <= self.obs_seq_len
        return self.decode(actions, self.encode(time, states))


def pack_ddpm_act_weights(net: EncDecDenoiser, n_timesteps: int) -> dict:
    """EncDecDenoiser in the operand order of csrc/policy_ddpm_act.h (width 64, obs <= 32, obs_seq_len <= 5, action_seq_len <= 4, A <= 8, linear head): every matrix
    through ``pack_tiles``; w_in = [tok_emb (columns padded to 32) | action_emb (columns padded to 16)]; the per-layer arrays enc_w, enc_v, dec_w, dec_v in the order of
    ``pack_act_weights``; head_w = action_pred (rows padded to 16); tab = [pos_emb (padded to 8 rows) | encoder.ln | decoder.ln | tok_emb bias | action_emb bias | head
    bias (padded to 16) | temb [T][64] = the module's own time_emb of steps 0 .. T-1 in f32 | sched [T][5] = ddpm_schedule of the cosine betas]."""
    assert net.embed_dim == 64 and net.state_dim <= 32 and net.action_dim <= 8 and net.obs_seq_len <= 5 and net.action_seq_len <= 4 and net.linear_output
    flat = lambda *xs: torch.cat([x.detach().to(torch.float32).reshape(-1) for x in xs])
    dev = net.pos_emb.device
    te = torch.zeros(64, 32, device=dev)
    te[:, :net.state_dim] = net.tok_emb.weight.detach()
    pos = torch.zeros(8, 64, device=dev)
    pos[:net.pos_emb.shape[1]] = net.pos_emb.detach()[0]
    hb = torch.zeros(16, device=dev)
    hb[:net.action_dim] = net.action_pred.bias.detach()
    enc_w, enc_v, dec_w, dec_v = [], [], [], []
    for b in net.encoder.blocks:
        a = b.attn
        enc_w.append(flat(*[pack_tiles(l.weight) for l in (a.query, a.key, a.value, a.proj, b.mlp[0], b.mlp[2])]))
        enc_v.append(flat(b.ln1.weight, b.ln2.weight, a.query.bias, a.key.bias, a.value.bias, a.proj.bias, b.mlp[0].bias, b.mlp[2].bias))
    for b in net.decoder.blocks:
        a = b.attn
        dec_w.append(flat(*[pack_tiles(l.weight) for l in (a.query, a.key, a.value, a.cross_query, a.cross_key, a.cross_value, a.proj, b.mlp[0], b.mlp[2])]))
        dec_v.append(flat(b.ln1.weight, b.ln2.weight, a.query.bias, a.key.bias, a.value.bias, a.cross_query.bias, a.cross_key.bias, a.cross_value.bias, a.proj.bias, b.mlp[0].bias, b.mlp[2].bias))
    temb = net.time_tokens(torch.arange(n_timesteps, device=dev))
    sched = ddpm_schedule(cosine_beta_schedule(n_timesteps).to(dev))["sched"]
    return {"w_in": flat(pack_tiles(te), pack_tiles(net.action_emb.weight)),
            "tab": flat(pos, net.encoder.ln.weight, net.decoder.ln.weight, net.tok_emb.bias, net.action_emb.bias, hb, temb, sched),
            "enc_w": torch.stack(enc_w), "enc_v": torch.stack(enc_v), "dec_w": torch.stack(dec_w), "dec_v": torch.stack(dec_v), "head_w": flat(pack_tiles(net.action_pred.weight))}


class DDPMACTPolicy(_ChunkLanes, NativePolicy):
    """DiffusionAgent.predict of the encoder-decoder agent without goals (agents/ddpm_encdec_agent.py:222-257) around Diffusion.sample (diffusion_policy.py:117-217)
    and DiffusionEncDec.forward (diffusion_models.py:844-905), on a batch: the scaled observation enters the lane's window (deque maxlen obs_seq_len S) on EVERY
    step; a lane whose ``counter`` equals the chunk length Ta is due and samples a new chunk of Ta actions from its window as it stands (L entries, 1 <= L <= S; the
    first step of an episode computes with L = 1): first iterate = noise, T reverse steps - epsilon prediction, x0 clipped to the data bounds in scaled space,
    posterior mean, posterior noise except at step 0 -, final clamp, inverse scaling as two f32 operations; every lane then emits chunk[counter] and counts on.
    ``reset()`` clears every window and makes all lanes due, ``begin_episodes(mask)`` the masked ones.

    All per-lane state lives on the device: ``counter``, ``chunk``, the window (``hist``, kept in place), its lengths, the step word.  On a HIP device the whole call
    is ONE kernel (csrc/policy_ddpm_act.h through d3il_ddpm_act_chunk_f32: width 64, 4 heads, obs <= 32, A <= 8, S <= 5, Ta <= 4, at most 4 encoder and 8 decoder
    layers, T <= 255, linear head) on the window in its ``padded()`` form, then a device-side add on the step word; lanes with different L and different counters
    run in one batch, and a call in which no lane of a 16-lane tile is due costs that tile only the emit.  On the CPU, for other shapes and with
    D3IL_POLICY_DDPM_ACT_FUSED=0 the same arithmetic runs as torch ops (``_chain_torch``, lanes grouped by L on the host) with the Philox normals computed on the
    host - that path cannot be captured.  Noise: Box-Muller on Philox4x32-10 keyed by ``seed`` with counter (env_offset + lane, step word, DDPM_ACT_TAG | k << 8 |
    j << 1 | q) - chain index k = T for the first iterate, i for reverse step i; index 0 is never drawn -, so results do not depend on batch order, sub-batches or
    ranks (``ddpm_act_normals`` is the host form); or ``noise_in(n) -> [n, T + 1, Ta, A]`` (index = chain index) when given (golden replay, tests).  A NaN / Inf in
    a due lane's valid window rows, head outputs or iterates marks the lane (``last_bad``) and gives it a NaN chunk (D3IL_FLAG_SOLVER_FAIL in that lane's steps)."""

    def __init__(self, model: EncDecDenoiser, scaler: Scaler, n_timesteps: int, obs_seq_len: int | None = None, seed: int = 0, n_envs: int | None = None, noise_in=None):
        self.model, self.scaler, self.T = model.eval(), scaler, int(n_timesteps)
        self.S = int(model.obs_seq_len if obs_seq_len is None else obs_seq_len)
        self.Ta, self.A, self.obs_dim = int(model.action_seq_len), int(model.action_dim), int(model.state_dim)
        assert 1 <= self.T <= 255 and 1 <= self.Ta <= 4 and 1 <= self.A <= 8, "the Philox counter layout holds T <= 255, chunks of at most 4 tokens and 8 components"
        assert 1 <= self.S <= model.obs_seq_len, "the window cannot exceed the denoiser's obs_seq_len"
        assert scaler.y_bounds is not None and tuple(scaler.y_bounds.shape) == (2, self.A), "DDPMACTPolicy clamps to the scaler's y_bounds"
        dev = scaler.x_mean.device
        self.device = dev
        self._sched = ddpm_schedule(cosine_beta_schedule(self.T).to(dev))["sched"]
        self._init_output(scaler)
        self._init_stream(seed)
        self.n_envs, self.noise_in = n_envs, noise_in
        self.counter = self.chunk = self.hist = self.last_bad = None      # per-lane state: i32 [N], f32 [N, Ta, A] (clamped, inverse-scaled), the window, i32 [N]
        self.record = False           # also keep the chunk table and what was drawn after every call (last_chunk, last_noise [N, T + 1, Ta, A]: zero where nothing was drawn)
        self.last_chunk = self.last_noise = None
        if n_envs is not None:
            self._state(int(n_envs))

    # ---- construction from the reference's objects
    @classmethod
    def from_reference(cls, agent, seed: int = 0, n_envs: int | None = None, device=None, noise_in=None):
        """From a live reference enc-dec ``DiffusionAgent`` (duck-typed) whose ``model`` is a ``Diffusion`` around a ``DiffusionEncDec``: the denoiser's state dict,
        ``n_timesteps``, ``agent.scaler``, ``agent.obs_seq_len``; with ``agent.use_ema`` the EMA shadow parameters (the reference swaps them in for every predict)."""
        diff = agent.model
        net = diff.model
        sd = {k: torch.as_tensor(v) for k, v in net.state_dict().items()}
        dev = torch.device(device) if device is not None else sd["tok_emb.weight"].device
        C, state_dim = sd["tok_emb.weight"].shape
        A, Ta = sd["action_emb.weight"].shape[1], int(net.action_seq_len)
        layers = lambda p: len({k.split(".")[2] for k in sd if k.startswith(p + ".blocks.")})
        den = EncDecDenoiser(state_dim, A, C, int(net.encoder.blocks[0].attn.n_head), layers("encoder"), layers("decoder"), sd["pos_emb"].shape[1] - Ta + 1, Ta,
                             int(net.encoder.blocks[0].attn.mask.shape[-1]), linear_output="action_pred.weight" in sd)
        own = den.state_dict()
        den.load_state_dict({k: sd[k].to(own[k].dtype) for k in own})
        pol = cls(den.to(dev).requires_grad_(False), Scaler.from_reference(agent.scaler, dev), int(diff.n_timesteps), obs_seq_len=int(agent.obs_seq_len), seed=seed,
                  n_envs=n_envs, noise_in=noise_in)
        if getattr(agent, "use_ema", False):
            pol.use_ema(agent.ema_helper.shadow_params)
        return pol

    @staticmethod
    def matches(agent) -> bool:
        """Is ``agent`` exactly what this policy restates: the reference's DiffusionAgent around a DiffusionEncDec without goals (``encoder`` / ``decoder`` stacks of one
        width, LayerNorms without bias, exact GELU, masks that cover 1 + obs_seq_len tokens), configured as the sampler restated here (``model.betas`` = the cosine
        schedule, epsilon prediction, clip_denoised, neither diffusion_x nor diffusion_kde)?  The GPT denoiser (``blocks``) and the MLP denoiser do not; everything
        else stays on the row-by-row adapter, which runs the reference's own code."""
        try:
            diff = agent.model
            net = diff.model
            if not all(hasattr(net, k) for k in ("encoder", "decoder", "time_emb", "action_emb", "tok_emb", "pos_emb", "action_pred", "state_dict")) or hasattr(net, "blocks"):
                return False
            if net.goal_conditioned is not False or getattr(agent, "goal_condition", False) or not hasattr(agent, "scaler") or agent.scaler.y_bounds is None:
                return False
            if getattr(diff, "diffusion_x", False) or getattr(agent, "diffusion_kde", False) or not getattr(diff, "predict_epsilon", True) or not getattr(diff, "clip_denoised", True):
                return False
            T = int(diff.n_timesteps)
            betas = torch.as_tensor(diff.betas).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
            if not (1 <= T <= 255 and betas.shape[0] == T and bool(torch.equal(betas, cosine_beta_schedule(T)))):
                return False
            C, Ta, S = int(net.tok_emb.out_features), int(agent.action_seq_size), int(agent.obs_seq_len)
            if Ta != int(net.action_seq_len) or not 1 <= Ta <= 4 or not 1 <= S <= int(net.obs_seq_len) or tuple(net.pos_emb.shape) != (1, int(net.obs_seq_len) - 1 + Ta, C):
                return False
            if net.tok_emb.bias is None or net.action_emb.bias is None or int(net.action_emb.out_features) != C or not 1 <= int(net.action_emb.in_features) <= 8:
                return False
            if not (isinstance(net.time_emb[1], nn.Linear) and isinstance(net.time_emb[2], nn.Mish) and isinstance(net.time_emb[3], nn.Linear)):
                return False
            if (net.time_emb[1].in_features, net.time_emb[1].out_features, net.time_emb[3].in_features, net.time_emb[3].out_features) != (C, 2 * C, 2 * C, C):
                return False
            heads = set()
            for stack, cross in ((net.encoder, False), (net.decoder, True)):
                if tuple(stack.ln.weight.shape) != (C,) or getattr(stack.ln, "bias", None) is not None or len(stack.blocks) < 1:
                    return False
                for b in stack.blocks:
                    a = b.attn
                    lins = [a.key, a.query, a.value, a.proj] + ([a.cross_key, a.cross_query, a.cross_value] if cross else [])
                    if hasattr(a, "cross_key") != cross or not all(isinstance(l, nn.Linear) and l.in_features == C and l.out_features == C and l.bias is not None for l in lins):
                        return False
                    if any(getattr(ln, "bias", None) is not None or tuple(ln.weight.shape) != (C,) for ln in (b.ln1, b.ln2)):
                        return False
                    if not (isinstance(b.mlp[0], nn.Linear) and isinstance(b.mlp[1], nn.GELU) and getattr(b.mlp[1], "approximate", "none") == "none" and isinstance(b.mlp[2], nn.Linear)):
                        return False
                    if (b.mlp[0].in_features, b.mlp[0].out_features, b.mlp[2].in_features, b.mlp[2].out_features) != (C, 4 * C, 4 * C, C):
                        return False
                    if a.mask.dim() != 4 or a.mask.shape[-1] != a.mask.shape[-2] or a.mask.shape[-1] < max(1 + int(net.obs_seq_len), Ta):
                        return False
                    heads.add(int(a.n_head))
            return len(heads) == 1 and C % heads.pop() == 0
        except (AttributeError, TypeError, ValueError, IndexError):
            return False

    # ---- the policy protocol of the Sims and SubBatchSet (NativePolicy; a fork and a capture keep the window, ``hist``, with the rest)
    SWITCH, STATE, LAST = "D3IL_POLICY_DDPM_ACT_FUSED", ("counter", "chunk", "last_bad"), ("last_chunk", "last_noise")
    TAKES = "the state tokens take %d"

    def _state(self, n):
        """counter / chunk / window / last_bad for n lanes; a new size starts with every lane due on an empty window."""
        if self.counter is None or self.counter.shape[0] != n:
            self._chunk_state(n, self.Ta)
            self.last_bad = torch.zeros(n, dtype=torch.int32, device=self.device)
            self.hist = _History(n, self.S, self.obs_dim, self.device)

    def load_reference_state_dict(self, sd):
        """``Diffusion.state_dict()`` of the reference: the denoiser sits under ``model.`` (a bare DiffusionEncDec state dict is taken as it is); masks are ignored."""
        if any(k.startswith("model.") for k in sd):
            sd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
        own = self.model.state_dict()
        self.model.load_state_dict({k: torch.as_tensor(sd[k]).to(own[k].dtype) for k in own})
        for p in self.model.parameters():
            p.requires_grad_(False)

    def _pack(self):
        return pack_ddpm_act_weights(self.model, self.T)

    # ---- the step
    def _kernel_shape(self) -> bool:
        m = self.model
        return (m.embed_dim == 64 and m.n_heads == 4 and 1 <= m.state_dim <= 32 and 1 <= m.action_dim <= 8 and 1 <= self.S <= 5 and m.obs_seq_len <= 5 and 1 <= self.Ta <= 4
                and 1 <= len(m.encoder.blocks) <= 4 and 1 <= len(m.decoder.blocks) <= 8 and 1 <= self.T <= 255 and m.linear_output)

    def _noise(self, n, dev, need_host: bool):
        """The normals [n, T + 1, Ta, A] (index = chain index; ``_draw``): in the host form index 0, which is never drawn, is zero."""
        def host(t):
            z = np.zeros((n, self.T + 1, self.Ta, self.A))
            for k in range(1, self.T + 1):
                z[:, k] = ddpm_act_normals(self.seed, self.env_offset, n, t, k, self.Ta, self.A)
            return z
        return self._draw(self.noise_in, n, (n, self.T + 1, self.Ta, self.A), host, need_host, dev)

    def _sched_for(self, dt, dev):
        if dt == torch.float32:
            return self._sched.to(dev)
        return ddpm_schedule(cosine_beta_schedule(self.T).to(device=dev, dtype=dt))["sched"]

    def _chain_torch(self, st, noise, x=None, k_start=None, k_stop=0):
        """A new chunk for every row of one window length: ``st`` [m, L, obs] (scaled), ``noise`` [m, T + 1, Ta, A]; in the dtype of ``st`` and the parameters (f32
        in the policy; the tests run it in f64 too), in the reference's order of operations.  ``x`` / ``k_start`` / ``k_stop``: only chain steps k_start .. k_stop
        from the given iterate.  Returns (chunk [m, Ta, A] clamped and inverse-scaled, NaN for marked rows; marked [m] bool; the last iterate before the final clamp)."""
        dt, dev = st.dtype, st.device
        c = lambda v: v.to(device=dev, dtype=dt)
        m, sched, lo, hi = self.model, self._sched_for(dt, dev), c(self.lo), c(self.hi)
        noise = c(noise)
        if x is None:
            x, k_start = noise[:, self.T], self.T - 1
        else:
            x = c(x)
        bad = ~torch.isfinite(st).reshape(st.shape[0], -1).all(dim=1) | ~torch.isfinite(x).reshape(st.shape[0], -1).all(dim=1)
        for i in range(k_start, k_stop - 1, -1):
            eps = m(x, torch.full((st.shape[0],), i, dtype=torch.long, device=dev), st)
            s = sched[i]
            x0 = torch.minimum(torch.maximum(s[0] * x - s[1] * eps, lo), hi)
            mean = s[2] * x0 + s[3] * x
            x = mean if i == 0 else mean + s[4] * noise[:, i]
            bad |= ~torch.isfinite(eps).reshape(st.shape[0], -1).all(dim=1) | ~torch.isfinite(x).reshape(st.shape[0], -1).all(dim=1)
        return self._action_tail(x, bad, False, lo, hi), bad, x

    def _push(self, s):
        """The scaled observation enters every lane's window: (window [N, S, obs] in its ``padded()`` form, lengths i64 [N])."""
        self.hist.append_(s)
        win, ln = self.hist.padded()
        return win.contiguous(), ln.contiguous()

    def _step_torch(self, s):
        win, ln = self._push(s)
        if win.is_cuda and _capturing():
            raise RuntimeError("DDPMACTPolicy: the torch path decides on the host which lanes are due, groups them by window length and draws its Philox numbers there; "
                               "it cannot be captured - the kernel can")
        n, dev = win.shape[0], win.device
        due = self._due()
        self.last_bad.zero_()
        if self.record:
            self.last_noise = torch.zeros(n, self.T + 1, self.Ta, self.A, dtype=torch.float32, device=dev)
        if bool(due.any()):
            noise = self._noise(n, dev, True)
            for L in torch.unique(ln[due]).tolist():
                rows = torch.nonzero(due & (ln == L)).reshape(-1)
                Lc = min(max(int(L), 1), self.S)
                y, bad, _ = self._chain_torch(win[rows, :Lc], noise[rows])
                self.chunk[rows] = y
                self.last_bad[rows] = bad.to(torch.int32)
            if self.record:
                drawn = noise.clone()
                drawn[:, 0] = 0
                self.last_noise.copy_(torch.where(due.reshape(-1, 1, 1, 1), drawn, self.last_noise))
            self.counter.masked_fill_(due, 0)
        return self._emit()

    def _step_kernel(self, s):
        from . import capi
        win, ln = self._push(s)
        n, dev, m = win.shape[0], win.device, self.model
        w = self._packed.current(self._pack_params(), self._pack)
        y = torch.empty(n, self.A, dtype=torch.float32, device=dev)
        noise_out = torch.zeros(n, self.T + 1, self.Ta, self.A, dtype=torch.float32, device=dev) if self.record else None
        assert ln.dtype == torch.int64
        capi.launch("d3il_ddpm_act_chunk_f32", dev, window=win, len=ln, **w, **self._draw_args(), noise_in=self._noise(n, dev, False), x_in=None, counter=self.counter,
                    chunk=self.chunk, actions=y, bad=self.last_bad, x_out=None, noise_out=noise_out, n_env=n, obs_dim=self.obs_dim, A=self.A, obs_seq_len=self.S,
                    action_seq_len=self.Ta, width=m.embed_dim, n_head=m.n_heads, n_enc=len(m.encoder.blocks), n_dec=len(m.decoder.blocks), n_timesteps=self.T,
                    linear_head=1, k_start=-1, k_stop=0)
        if self.record:
            self.last_noise = noise_out
        return y

    def _fallback_text(self):
        return ("this network (width %d, %d heads, window %d, chunk %d, linear head %s) is not one the chain kernel is built for; every call "
                "runs the torch path with a device synchronisation per call and no graph capture"
                % (self.model.embed_dim, self.model.n_heads, self.S, self.Ta, self.model.linear_output))

    @classmethod
    def random(cls, obs_dim: int, action_dim: int, device="cuda", seed: int = 0, obs_seq_len: int = 5, action_seq_len: int = 4, n_timesteps: int = 16, enc_layers: int = 2,
               dec_layers: int = 4, embed_dim: int = 64, n_heads: int = 4, window_size: int = 8, action_scale: float = 0.002, bound: float = 1.5, policy_seed: int = 0,
               linear_output: bool = True, **kw):
        """A policy of the reference's shape (configs/agents/ddpm_encdec_agent.yaml: 2 encoder and 4 decoder layers, width 64, 4 heads, obs_seq_len 5, chunks of 4, 16
        timesteps, masks of window_size + 1) with the fixed trained-like weights of ``ddpm_act_synthetic_state`` (there are no checkpoints offline), unit
        observation scaling, actions of ``action_scale`` per unit of the scaled space, bounds +-``bound``."""
        net = EncDecDenoiser(obs_dim, action_dim, embed_dim, n_heads, enc_layers, dec_layers, obs_seq_len, action_seq_len, max(window_size + 1, 1 + obs_seq_len, action_seq_len),
                             linear_output=linear_output)
        net.load_state_dict({k: torch.as_tensor(v) for k, v in ddpm_act_synthetic_state({k: v.shape for k, v in net.state_dict().items()}, seed).items()})
        return cls(net.requires_grad_(False).to(device), Scaler.unit(obs_dim, action_dim, action_scale, bound, device), n_timesteps, seed=policy_seed, **kw)
