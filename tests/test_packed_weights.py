"""policies.PackedWeights - the one cache behind the packed device copies of _Block, FusedResMLP and DDPMPolicy - and the one residual-MLP packer."""
import copy

import pytest
import torch

from d3il_amd import policies as P


def _same(got: dict, want: dict):
    for k, v in want.items():
        assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k


def _ptrs(buf: dict):
    return {k: v.data_ptr() for k, v in buf.items() if torch.is_tensor(v)}


class _BlockUser:
    packer = "pack_mlp_weights_f16x3"      # called once per pack

    def __init__(self):
        self.m = P._Block(120, 6, 11)

    def ensure(self):
        self.m.ensure_packed()

    def invalidate(self):
        self.m.invalidate_packed()

    def buf(self):
        return self.m._packed.buf

    def weights(self):
        return [self.m.attn.query.weight, self.m.attn.proj.weight, self.m.attn.value.bias, self.m.mlp[2].weight]

    def fresh(self):
        a, fc1, fc2 = self.m.attn, self.m.mlp[0], self.m.mlp[2]
        wq = torch.cat((a.query.weight, a.key.weight, a.value.weight), dim=0)
        hq, hp = P.pack_linear120_weights_f16x3(wq), P.pack_linear120_weights_f16x3(a.proj.weight)
        return {"wp_qkv": P.pack_linear120_weights(wq), "wp_proj": P.pack_linear120_weights(a.proj.weight), "wp_mlp": P.pack_mlp_weights(fc1, fc2),
                "b_qkv": torch.cat((a.query.bias, a.key.bias, a.value.bias)), "hp_qkv": hq, "hp_proj": hp, "hp_mlp": P.pack_mlp_weights_f16x3(fc1.weight, fc2.weight),
                "hp_attn": torch.cat((hq, hp)), "w_oor": torch.zeros((), dtype=torch.int64)}


class _ResMLPUser:
    packer = "pack_resmlp_weights"

    def __init__(self):
        self.m = P.ResidualMLP(10, 128, 6, 2)
        self.m._fused = P.FusedResMLP()

    def ensure(self):
        self.m._fused.ensure_packed(self.m._parts())

    def invalidate(self):
        self.m.invalidate_packed()

    def buf(self):
        return self.m._fused._packed.buf

    def weights(self):
        return [self.m.layers[0].weight, self.m.layers[2].l2.weight, self.m.layers[-1].bias]

    def fresh(self):
        return P.pack_resmlp_weights(*self.m._parts())


class _DDPMUser:
    packer = "pack_resmlp_weights"

    def __init__(self):
        sc = P.Scaler([0.0] * 16, [1.0] * 16, [0.0, 0.0], [1.0, 1.0], y_bounds=[[-1.0, -1.0], [1.0, 1.0]], device="cpu")
        self.m = P.DDPMPolicy(P.DiffusionMLP(2, 16, 8, 256, 2), sc, 4, 1)

    def ensure(self):
        self.m.ensure_packed()

    def invalidate(self):
        self.m.invalidate_packed()

    def buf(self):
        return self.m._packed.buf

    def weights(self):
        net = self.m.model
        return [net.layers.layers[0].weight, net.layers.layers[1].l1.bias, net.temp_layers[1].weight]

    def fresh(self):
        net = self.m.model
        with torch.no_grad():
            return dict(P.pack_resmlp_weights(*net.layers._parts()), temb=net.temp_layers(torch.arange(4)).to(torch.float32))


@pytest.mark.parametrize("user", [_BlockUser, _ResMLPUser, _DDPMUser])
def test_cache_follows_the_parameters_in_place(user, monkeypatch):
    torch.manual_seed(1)
    u = user()
    calls = []
    real = getattr(P, u.packer)
    monkeypatch.setattr(P, u.packer, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    u.ensure()
    ptrs = _ptrs(u.buf())
    assert len(calls) == 1 and len(ptrs) >= 6
    assert not set(ptrs.values()) & {p.data_ptr() for p in getattr(u.m, "model", u.m).parameters()}      # the cache owns its buffers: no view of a parameter
    _same(u.buf(), u.fresh())
    assert not any(k.startswith("_packed") or "_fused" in k for k in getattr(u.m, "model", u.m).state_dict())      # a plain attribute: checkpoints load by name
    # (a) unchanged parameters: no pack, same buffers
    n = len(calls)
    u.ensure()
    assert len(calls) == n and _ptrs(u.buf()) == ptrs
    # (b) an in-place change is seen through the version counters and lands in the SAME buffers
    with torch.no_grad():
        for w in u.weights():
            w.mul_(1.5)
    before = {k: v.clone() for k, v in u.buf().items() if torch.is_tensor(v)}
    u.ensure()
    assert _ptrs(u.buf()) == ptrs
    _same(u.buf(), u.fresh())
    assert sum(not torch.equal(before[k], u.buf()[k]) for k in before) >= 2
    # (c) invalidate: the next ensure packs again (still in place)
    n = len(calls)
    u.ensure()
    assert len(calls) == n
    u.invalidate()
    u.ensure()
    assert len(calls) > n and _ptrs(u.buf()) == ptrs
    # (d) a deep copy owns its buffers and follows ITS weights
    twin = copy.deepcopy(u)
    want_orig = {k: v.clone() if torch.is_tensor(v) else v for k, v in u.buf().items()}
    tp = _ptrs(twin.buf())
    assert set(tp) == set(ptrs) and all(tp[k] != ptrs[k] for k in ptrs)
    with torch.no_grad():
        for w in twin.weights():
            w.mul_(0.5)
    twin.ensure()
    _same(twin.buf(), twin.fresh())
    u.ensure()
    _same(u.buf(), want_orig)
    assert _ptrs(u.buf()) == ptrs and _ptrs(twin.buf()) == tp


def test_cache_replaces_buffers_whose_layout_changed():
    """Names, shapes, dtypes and devices decide between the in-place copy and new buffers."""
    c = P.PackedWeights()
    p = [torch.zeros(3)]
    c.ensure(p, lambda: {"a": torch.ones(3), "n": 1})
    a = c.buf["a"]
    p[0].add_(1)
    c.ensure(p, lambda: {"a": torch.full((3,), 2.0), "n": 2})
    assert c.buf["a"] is a and a.tolist() == [2.0] * 3 and c.buf["n"] == 2
    for other in (torch.ones(3, device="meta"), torch.ones(3), torch.ones(3, dtype=torch.float64), torch.ones(4, dtype=torch.float64)):      # device, device, dtype, shape
        p[0].add_(1)
        c.ensure(p, lambda: {"a": other, "n": 2})
        assert c.buf["a"] is not a and (c.buf["a"].shape, c.buf["a"].dtype, c.buf["a"].device) == (other.shape, other.dtype, other.device)
        a = c.buf["a"]
    p[0].add_(1)
    c.ensure(p, lambda: {"b": torch.ones(3, dtype=torch.float64), "n": 2})
    assert set(c.buf) == {"b", "n"}


@pytest.mark.parametrize("hidden", [128, 256])
def test_resmlp_packer_layout(hidden):
    """pack_resmlp_weights against its docstring, position by position: [T_out][t][16 g + i][r] = W[16 T_out + i][16 t + 4 g + r] for the square layers and the
    output layer (rows padded to 16), [T_out][16 g + i][s] = W[16 T_out + i][4 s + g] for the input layer (columns padded to 32: step s of k_resmlp_f32's first
    product takes input feature 4 s + g), zeros beyond the matrices."""
    torch.manual_seed(hidden)
    IN, OUT, NB = 13, 3, 2
    lin_in, lin_out = torch.nn.Linear(IN, hidden), torch.nn.Linear(hidden, OUT)
    blocks = [(torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, hidden)) for _ in range(NB)]
    fw = P.pack_resmlp_weights(lin_in, blocks, lin_out)
    NT = hidden // 16
    assert fw["n_blocks"] == NB and tuple(fw["w_in"].shape) == (NT, 64, 8) and tuple(fw["w_blk"].shape) == (2 * NB, NT, NT, 64, 4)
    assert tuple(fw["w_out"].shape) == (NT, 64, 4) and tuple(fw["b_out"].shape) == (16,) and tuple(fw["b_blk"].shape) == (2 * NB, hidden)
    layers = [l for b in blocks for l in b]
    for l in layers + [lin_in, lin_out]:
        l.requires_grad_(False)
    g_ = torch.Generator().manual_seed(7)
    draw = lambda hi: int(torch.randint(hi, (1,), generator=g_))
    nonzero = 0
    for _ in range(300):
        l, To, t, g, i, r, s = draw(2 * NB), draw(NT), draw(NT), draw(4), draw(16), draw(4), draw(8)
        assert float(fw["w_blk"][l, To, t, 16 * g + i, r]) == float(layers[l].weight[16 * To + i, 16 * t + 4 * g + r])
        want = float(lin_out.weight[i, 16 * t + 4 * g + r]) if i < OUT else 0.0
        assert float(fw["w_out"][t, 16 * g + i, r]) == want
        col = 4 * s + g
        want = float(lin_in.weight[16 * To + i, col]) if col < IN else 0.0
        assert float(fw["w_in"][To, 16 * g + i, s]) == want
        nonzero += want != 0.0
    assert nonzero > 50
    for k in range(16):
        assert float(fw["b_out"][k]) == (float(lin_out.bias[k]) if k < OUT else 0.0)
    assert torch.equal(fw["b_in"], lin_in.bias.detach()) and torch.equal(fw["b_blk"], torch.stack([l.bias for l in layers]).detach())


@pytest.mark.gpu
def test_block_packed_on_the_cpu_follows_the_module_to_the_device(monkeypatch):
    """A block packed on the CPU and then moved: every packed buffer - the split-f16 ones too - is on the device BEFORE a kernel sees it."""
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    blk = P._Block(120, 6, 11).eval()
    blk.ensure_packed()
    assert all(v.device.type == "cpu" for v in blk._packed.buf.values())
    blk.to(dev)
    blk.ensure_packed()
    assert len(blk._packed.buf) == 9 and all(v.device == dev for v in blk._packed.buf.values())
    x = torch.randn(2, 11, 120, device=dev).contiguous()
    outs = {}
    with torch.no_grad():
        for mode in ("f16x3", "f32"):
            monkeypatch.setenv("D3IL_POLICY_GEMM", mode)
            outs[mode] = blk(x)
        monkeypatch.setenv("D3IL_POLICY_FUSED_MLP", "0")
        ref = blk(x)
    for mode in ("f16x3", "f32"):
        err = float((outs[mode] - ref).abs().max()) / float(ref.abs().max())
        assert err < 2e-5, (mode, err)
