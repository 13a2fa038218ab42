"""d3il_gpt_trunk72_f16x3 (csrc/policy_trunk72.h: the whole block chain of a 72-wide, 4-head transformer trunk in one launch) through its C entry, against an f64
restatement written out here with torch ops on the CPU.

The bar is the rule of tests/test_gpu_f16x3_edges.py:   err_kernel <= 4 x yardstick + sites x 2^-24 x max |want|
  yardstick: the same restatement in f32 on the device (torch's own layers on the same rows), taken per case and never carried over;
  sites: one layer has s = 2 split sites that do not pass through a LayerNorm (the attention output, the GELU output): 4 + 4 s = 12; the four-layer cases use
     4 + 8 n_layer, which assumes that the case's blocks do not amplify (the measured multiples are in profiles/trunk72/README.md).
One wave owns one 16-row tile = floor(16 / T) whole sequences; a workgroup has four tiles below 2048 tiles per launch and eight from there on, so the shapes are
1 sequence, exactly one tile, one tile plus one sequence, one (four-wave) workgroup plus one sequence, 130, and one launch at 2049 tiles for the eight-wave
instantiation.  Every output sits in a Guarded buffer of the f32 edge suite (sentinel bands in front and behind, the interior pre-filled).  All inputs and
references are built on the CPU; tests/test_policies_trunk72.py::test_the_inputs_do_their_job (no GPU) keeps a later change of seed or shape from emptying a test."""
import copy
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_policy_f32_edges as f32e      # noqa: E402  (Guarded, shifted, bits; a module, so nothing of it is collected here)

gpu = pytest.mark.gpu
Guarded, shifted, SENT = f32e.Guarded, f32e.shifted, f32e.SENT
EINVAL, EUNSUPPORTED = -1, -5
U = 2.0 ** -24
C, NH, D, HID = 72, 4, 18, 288
ATT_SCALE = {"randn": 1.0, "sharp": 10.0, "flat": 2.0 ** -6}      # query and key weights and biases times this: the scores go with its square
T_ALL = (1, 3, 5, 11, 16)
WG_TILES, WIDE_TILES = 4, 2048


def seq_counts(T):
    """1, exactly one tile, one tile plus one sequence, one workgroup plus one sequence, 130 (duplicates dropped, order kept)."""
    spt = 16 // T
    return list(dict.fromkeys((1, spt, spt + 1, WG_TILES * spt + 1, 130)))


ACC_CASES = [(n, T) for T in T_ALL for n in seq_counts(T)]
WIDE_CASES = [(WIDE_TILES * (16 // T) + 1, T) for T in (3, 11)]      # 2049 tiles: the eight-wave instantiation, its last workgroup with seven dead waves
CHAIN_CASES = [(6, 3), (3, 11)]
DEEP_CASES = [(130, 3), (17, 11)]
INDEP_T = (3, 11)
NAN_CASE = dict(n_seq=7, T=3, seq=2, tok=1, col=5)
CLIP_CASE = dict(n_seq=7, T=3, seq=4, tok=2, col=9, unit=100, big=1.0e6)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def blocks_of(seed, n_layer, att="randn"):
    """n_layer blocks (72, 4 heads, 288) with torch's default initialisation (what the policies' .random() draws), LayerNorm weights and biases moved off 1 / 0,
    on the CPU; the query and key layers times ATT_SCALE[att]."""
    from d3il_amd import policies as P
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        blocks = torch.nn.Sequential(*[P._Block(C, NH, 16) for _ in range(n_layer)])
    g = gen(seed + 1)
    with torch.no_grad():
        for blk in blocks:
            for ln in (blk.ln1, blk.ln2):
                ln.weight.copy_(1.0 + 0.2 * torch.randn(C, generator=g))
                ln.bias.copy_(0.1 * torch.randn(C, generator=g))
            for lin in (blk.attn.query, blk.attn.key):
                lin.weight.mul_(ATT_SCALE[att])
                lin.bias.mul_(ATT_SCALE[att])
    return blocks.requires_grad_(False)


def restate(blocks, x, dtype, device, sites=None):
    """The chain written out with torch ops in ``dtype`` on ``device``: x [n_seq, T, 72] -> [n_seq, T, 72].  sites (a list): gets, per layer, the operands of the four
    split sites (LN1 row, attention output, LN2 row, GELU output)."""
    F = torch.nn.functional
    cv = lambda t: t.detach().to(device=device, dtype=dtype)
    x = cv(x)
    n, T, _ = x.shape
    mask = torch.ones(T, T, dtype=torch.bool, device=device).tril()
    for blk in blocks:
        a = blk.attn
        eps = blk.ln1.eps
        h = F.layer_norm(x, (C,), cv(blk.ln1.weight), cv(blk.ln1.bias), eps)
        q, k, v = (F.linear(h, cv(l.weight), cv(l.bias)).view(n, T, NH, D).transpose(1, 2) for l in (a.query, a.key, a.value))
        att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(D))
        att = att.masked_fill(~mask, float("-inf"))
        y = (torch.softmax(att, dim=-1) @ v).transpose(1, 2).reshape(n, T, C)
        x = x + F.linear(y, cv(a.proj.weight), cv(a.proj.bias))
        h2 = F.layer_norm(x, (C,), cv(blk.ln2.weight), cv(blk.ln2.bias), blk.ln2.eps)
        u = F.linear(h2, cv(blk.mlp[0].weight), cv(blk.mlp[0].bias))
        ge = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
        if sites is not None:
            sites.append((h, y, h2, ge))
        x = x + F.linear(ge, cv(blk.mlp[2].weight), cv(blk.mlp[2].bias))
    return x


def rows_of(seed, n_seq, T):
    return torch.randn(n_seq, T, C, generator=gen(seed))


def within(tag, got, want, yard_out, sites):
    """Print kernel / torch f32 / multiple (and the share of the bound used), then the one assertion of every comparison."""
    err, yard, mag = float((got.double() - want).abs().max()), float((yard_out.double().cpu() - want).abs().max()), float(want.abs().max())
    bound = 4 * yard + sites * U * mag
    print("%s: kernel %.3e / torch f32 %.3e / multiple %.2f / of its bound %.3f" % (tag, err, yard, err / max(yard, 1e-300), err / max(bound, 1e-300)))
    assert err <= bound, tag


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


_PACKS = {}


def packed(dev, blocks):
    """The chain's packed stream and vectors on the device, packed once per chain."""
    from d3il_amd import policies as P
    if id(blocks) not in _PACKS:
        pk = P.pack_trunk72_weights(blocks)
        _PACKS[id(blocks)] = (blocks, pk["w"].to(dev), pk["vec"].to(dev))
    return _PACKS[id(blocks)][1:]


def launch(dev, blocks, x, layers=None, xd=None):
    """d3il_gpt_trunk72_f16x3 on a device copy of the CPU tensor x (or on the device tensor xd), the output guarded; layers = (first, count) of the chain."""
    from d3il_amd import capi
    w, vec = packed(dev, blocks)
    first, count = layers if layers else (0, len(blocks))
    xd = x.to(torch.float32).contiguous().to(dev) if xd is None else xd
    out = Guarded(dev, tuple(xd.shape))
    rc = capi.load().d3il_gpt_trunk72_f16x3(xd.data_ptr(), w[first].data_ptr(), vec[first].data_ptr(), float(blocks[0].ln1.eps), out.ptr, xd.shape[0], xd.shape[1], count, stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and w is not None and vec is not None
    return out.read()


def bits(t):
    return t.contiguous().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. one layer, accuracy
def accuracy(dev, tag, blocks, x, sites):
    want = restate(blocks, x, torch.float64, "cpu")
    yard = restate(blocks, x, torch.float32, dev)
    within(tag, launch(dev, blocks, x), want, yard, sites)


@gpu
@pytest.mark.parametrize("n_seq,T", ACC_CASES + WIDE_CASES)
def test_one_layer_matches_f64(dev, n_seq, T):
    accuracy(dev, "trunk72 1 layer n_seq %d T %d" % (n_seq, T), blocks_of(11, 1), rows_of(100 + T, n_seq, T), 12)


@gpu
@pytest.mark.parametrize("att", ["sharp", "flat"])
def test_one_layer_attention_scales(dev, att):
    accuracy(dev, "trunk72 1 layer %s T 11" % att, blocks_of(12, 1, att), rows_of(7, 9, 11), 12)


# ------------------------------------------------------------------------------------------------ 2. chaining is exact
@gpu
@pytest.mark.parametrize("n_seq,T", CHAIN_CASES)
def test_four_layers_in_one_launch_equal_four_launches(dev, n_seq, T):
    blocks = blocks_of(13, 4)
    x = rows_of(21, n_seq, T)
    one = launch(dev, blocks, x)
    step = x
    for l in range(4):
        step = launch(dev, blocks, step, layers=(l, 1))
    assert (bits(one) == bits(step)).all()


# ------------------------------------------------------------------------------------------------ 3. four layers against f64
@gpu
@pytest.mark.parametrize("n_seq,T", DEEP_CASES)
def test_four_layers_match_f64(dev, n_seq, T):
    accuracy(dev, "trunk72 4 layers n_seq %d T %d" % (n_seq, T), blocks_of(13, 4), rows_of(31 + T, n_seq, T), 4 + 8 * 4)


# ------------------------------------------------------------------------------------------------ 4. row independence
@gpu
@pytest.mark.parametrize("T", INDEP_T)
def test_sequences_are_independent(dev, T):
    blocks = blocks_of(13, 4)
    x = rows_of(41 + T, 130, T)
    full = launch(dev, blocks, x)
    perm = torch.randperm(130, generator=gen(5))
    assert (bits(launch(dev, blocks, x[perm])) == bits(full[perm])).all(), "permuting the sequences permutes the output"
    for s in (0, 7, 129):
        assert (bits(launch(dev, blocks, x[s:s + 1])) == bits(full[s:s + 1])).all(), "sequence %d alone" % s


# ------------------------------------------------------------------------------------------------ 5. guard
def nan_input():
    c = NAN_CASE
    x = rows_of(51, c["n_seq"], c["T"])
    bad = x.clone()
    bad[c["seq"], c["tok"], c["col"]] = float("nan")
    return x, bad


def clip_case():
    """One block and rows where exactly ONE row has a split-site operand beyond 65504 (about 7e4): the row holds one huge feature, so LN2 of it is nearly one-hot
    (sqrt(71) ln2.weight at that feature), and one fc1 row weighs that feature by 7e4 / that value - the row's GELU output of that unit is the operand."""
    c = CLIP_CASE
    blocks = torch.nn.Sequential(*[copy.deepcopy(blocks_of(14, 1)[0])])
    x = rows_of(52, c["n_seq"], c["T"])
    x[c["seq"], c["tok"], c["col"]] = c["big"]
    with torch.no_grad():
        blk = blocks[0]
        blk.ln2.weight[c["col"]] = 1.0
        blk.ln2.bias[c["col"]] = 0.0
        blk.mlp[0].weight[c["unit"]] = 0.0
        blk.mlp[0].weight[c["unit"], c["col"]] = 7.0e4 / math.sqrt(71.0)
        blk.mlp[0].bias[c["unit"]] = 0.0
    return blocks, x


@gpu
def test_guard_nan_stays_in_its_sequence(dev):
    from d3il_amd import policies as P
    c = NAN_CASE
    blocks = blocks_of(13, 4)
    x, bad = nan_input()
    with P.RangeGuard(dev) as guard:
        clean = launch(dev, blocks, x)
        assert guard.read() == {"clipped": 0, "nonfinite": 0, "launches": 1}
        guard.reset()
        got = launch(dev, blocks, bad)
        rep = guard.read()
    assert torch.isnan(got[c["seq"], c["tok"]:]).all(), "the NaN token and the later tokens of its sequence are NaN in every column"
    keep = torch.ones(c["n_seq"], c["T"], dtype=torch.bool)
    keep[c["seq"], c["tok"]:] = False
    assert (bits(got[keep]) == bits(clean[keep])).all(), "token 0 of the sequence and every other sequence are those of a clean launch"
    assert rep == {"clipped": 0, "nonfinite": c["T"] - c["tok"], "launches": 1}
    assert (bits(launch(dev, blocks, x)) == bits(clean)).all(), "the guarded and the default instantiation agree on clean rows"


@gpu
def test_guard_counts_a_clipped_row_once(dev):
    from d3il_amd import policies as P
    blocks, x = clip_case()
    plain = launch(dev, blocks, x)
    with P.RangeGuard(dev) as guard:
        got = launch(dev, blocks, x)
        rep = guard.read()
    assert rep == {"clipped": 1, "nonfinite": 0, "launches": 1}
    assert torch.isfinite(got).all() and (bits(got) == bits(plain)).all(), "saturation is the same with and without the guard"


# ------------------------------------------------------------------------------------------------ 6. refusals
@gpu
def test_refusals_leave_the_output_untouched(dev):
    from d3il_amd import capi
    blocks = blocks_of(11, 1)
    w, vec = packed(dev, blocks)
    lib = capi.load()
    x = rows_of(61, 3, 5).to(dev)
    out = Guarded(dev, (3, 5, C))
    call = lambda xp, T, nl, n=3: lib.d3il_gpt_trunk72_f16x3(xp, w.data_ptr(), vec.data_ptr(), 1e-5, out.ptr, n, T, nl, stream(dev))
    assert call(x.data_ptr(), 0, 1) == EUNSUPPORTED and call(x.data_ptr(), 17, 1) == EUNSUPPORTED
    assert call(x.data_ptr(), 5, 0) == EUNSUPPORTED and call(x.data_ptr(), 5, 9) == EUNSUPPORTED and call(x.data_ptr(), 5, 1, 0) == EUNSUPPORTED
    keepalive, xp = shifted(dev, x.cpu(), 1)
    assert xp % 16 != 0 and call(xp, 5, 1) == EINVAL
    assert call(out.ptr, 5, 1) == EINVAL, "out must not alias x"
    assert b"d3il_gpt_trunk72_f16x3" in lib.d3il_last_error()
    torch.cuda.synchronize(dev)
    assert (out.bits() == SENT.view(np.uint32)).all() and keepalive is not None
