"""The three split-f16 policy kernels of csrc/policy_f16x3.h - k_linear120_f16x3, k_mlp_gelu_residual_f16x3, k_attn_half_f16x3 - through their C entries
(d3il_linear120_f16x3, d3il_mlp_ln_gelu_residual_f16x3, d3il_attn_half_f16x3; the range guard off: the default instantiations) against f64 restatements written
out here with torch f64 ops, at the shapes, operand scales and edges tests/test_policies_f16x3.py never runs.

Every comparison (within):   err_kernel <= 4 x yardstick + (4 + 4 s) x 2^-24 x max |want| + floor
  yardstick: torch's own f32 layers on the same rows on the same device, taken per case and never carried over (the factor 4 is that of the f32 edge suite);
  s: the split sites between input and output that do not pass through a LayerNorm - 1 for the linear entry without LayerNorm (0 with it), 1 for the MLP (the GELU
     output), 1 for the attention half (the attention output).  A split operand carries 22 bits: hi = RN11(x) leaves at most 2^-11 |x|, lo = RN11(resid 2^11)
     leaves at most 2^-22 |x| = 4 x 2^-24 |x| - four f32 roundings per site;
  floor = 2^-36 max_(r, n) (sum_k |W[n, k]| + sum_k |x[r, k]|): operands whose low half is a subnormal f16 (absolute step 2^-24 / 2^11, half of it the rounding).
     Applied to the linear entry (groups 1 - 3: it matters in the scale sweep only); the MLP and attention cases run at O(1) operands with floor = 0.
Cases are homogeneous in row scale, so the batch-wide max |want| hides nothing; the saturated rows of group 3 are judged one by one.  Every output sits in the middle
of a larger buffer (Guarded, of the f32 edge suite): 64 sentinel floats in front and behind must be bit-unchanged, the interior is pre-filled with the sentinel and
none of it may survive.  All references and input conditions are built on the CPU; test_the_inputs_do_their_job (no GPU) keeps a later change of seed or shape from
quietly emptying a test.  One wave handles 16 rows, one workgroup 64 (the attention half: one wave per sequence, 8 or 4 per workgroup)."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_policy_f32_edges as f32e      # noqa: E402  (Guarded, shifted, bits, attention; a module, so nothing of it is collected here)

gpu = pytest.mark.gpu
Guarded, shifted, bits, SENT = f32e.Guarded, f32e.shifted, f32e.bits, f32e.SENT
EINVAL, EUNSUPPORTED = -1, -5
U = 2.0 ** -24
SAT = 65504.0
ROWS = 33
LIN_ROWS = (1, 15, 16, 17, 63, 64, 65, 129)
LIN_N = (4, 20, 32, 36, 120, 360, 384)      # one padded tile; a tile cut by col < N; exactly one LDS stage; an odd tile count; the two shipped sizes; the bias table full
LIN_FORMS = {"plain": (None, False), "resid": (None, True), "ln1e-5": (1e-5, False), "ln1e-3": (1e-3, False), "ln1e-5_resid": (1e-5, True), "ln1e-3_resid": (1e-3, True)}
LIN_PAIRS = [(r, LIN_N[i % len(LIN_N)]) for i, r in enumerate(LIN_ROWS)]      # every row count and every N, in each form
SWEEP_E = (-20, -16, -12, -8, 0, 8, 14)
SWEEP = [("x", e) for e in SWEEP_E] + [("w", e) for e in SWEEP_E if e != 0]      # rows times 2^e; the weights times 2^e under rows at e = 0 (2^-12 among them)
SAT_VALUES = (65504.0, 65505.0, 7e4, 1e30, 3.4e38, float("inf"), -65504.0, -65505.0, -7e4, -1e30, -3.4e38, float("-inf"))
SAT_ROWS, SAT_COLS = (3, 20, ROWS - 1), (7, 119, 0)      # waves 0, 1, 2 of the workgroup; row 32 is the last live row, the one the dead lanes re-read
MLP_ROWS = (1, 16, 17, 64, 65, 129)
GAINS = (1, 4)
BANDS = ((-12, -8), (-8, -5), (-5, -1.5), (-1.5, -1.3), (-1.3, -1e-3), (-1e-3, 1e-3), (1e-3, 1.3), (1.3, 1.5), (1.5, 5), (5, 12), (12, 1000))
GELU_ROWS = 129
ATT_CASES = [(9 if T <= 11 else 5, T) for T in range(1, 17)] + [(1, 11), (1, 16)]
ATT_SCALE = {"randn": 1.0, "sharp": 10.0, "flat": 2.0 ** -6}      # query and key weights and biases times this: the scores go with its square
NF_ROWS = 37      # the guard suite's padded shapes: a partly filled third wave and a dead fourth one; both attention instantiations with dead waves
NF_ATT = [(3, 11), (5, 16)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def guard_off(monkeypatch):
    """These are the default (GUARD = false) instantiations: no guard is active before or after any test here."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_RANGE_GUARD", raising=False)
    assert P.range_guard() is None
    yield
    assert P.range_guard() is None


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ln64(x, w, b, eps):
    """nn.LayerNorm over the last axis (biased variance) in f64."""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def floor_of(W, x):
    return 2.0 ** -36 * (float(W.double().abs().sum(dim=1).max()) + float(x.double().abs().sum(dim=1).max()))


def within(tag, got, want, yard_out, s, floor=0.0):
    """Print kernel / torch f32 / multiple (and the share of the bound used), then the one assertion of every comparison."""
    err, yard, mag = float((got.double() - want).abs().max()), float((yard_out.double().cpu() - want).abs().max()), float(want.abs().max())
    bound = 4 * yard + (4 + 4 * s) * U * mag + floor
    print("%s: kernel %.3e / torch f32 %.3e / multiple %.2f / of its bound %.3f" % (tag, err, yard, err / max(yard, 1e-300), err / max(bound, 1e-300)))
    assert err <= bound, tag


def ptr(t):
    return None if t is None else t.data_ptr()


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def to_dev(dev, *ts):
    return [None if t is None else t.to(torch.float32).contiguous().to(dev) for t in ts]


# ------------------------------------------------------------------------------------------------ launches (every pointer handed over is alive until the result is read)
def linear_launch(dev, x, W, bias, resid=None, ln=None):
    """d3il_linear120_f16x3 on device copies of CPU tensors, the output guarded; ln = (weight, bias, eps) or None."""
    from d3il_amd import capi, policies as P
    rows, N = x.shape[0], W.shape[0]
    xd, bd, rd, lw, lb = to_dev(dev, x, bias, resid, *(ln[:2] if ln else (None, None)))
    wp = P.pack_linear120_weights_f16x3(W.to(torch.float32)).to(dev)
    out = Guarded(dev, (rows, N))
    rc = capi.load().d3il_linear120_f16x3(xd.data_ptr(), ptr(lw), ptr(lb), float(ln[2]) if ln else 0.0, wp.data_ptr(), bd.data_ptr(), ptr(rd), out.ptr, rows, N, stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and wp is not None
    return out.read()


def mlp_launch(dev, h, x, W1, b1, W2, b2, ln=None):
    """d3il_mlp_ln_gelu_residual_f16x3; x = None: the shipped call, the residual is the very buffer of h."""
    from d3il_amd import capi, policies as P
    rows = h.shape[0]
    hd, xd, b1d, b2d, lw, lb = to_dev(dev, h, x, b1, b2, *(ln[:2] if ln else (None, None)))
    wp = P.pack_mlp_weights_f16x3(W1.to(torch.float32), W2.to(torch.float32)).to(dev)
    out = Guarded(dev, (rows, 120))
    rc = capi.load().d3il_mlp_ln_gelu_residual_f16x3(hd.data_ptr(), ptr(lw), ptr(lb), float(ln[2]) if ln else 0.0, hd.data_ptr() if xd is None else xd.data_ptr(), wp.data_ptr(),
                                                     b1d.data_ptr(), b2d.data_ptr(), out.ptr, rows, 120, 480, stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and wp is not None
    return out.read()


def attn_pack(a):
    from d3il_amd import policies as P
    wqkv = torch.cat((a["wq"], a["wk"], a["wv"]), 0).contiguous()
    wp = torch.cat((P.pack_linear120_weights_f16x3(wqkv), P.pack_linear120_weights_f16x3(a["wp"])), 0).contiguous()
    assert tuple(wp.shape) == (32, 512, 8)
    return wp, torch.cat((a["bq"], a["bk"], a["bv"]), 0).contiguous()


def attn_launch(dev, a, x):
    """d3il_attn_half_f16x3 on x [B, T, 120] with the parameters a (attn_params)."""
    from d3il_amd import capi
    B, T, _ = x.shape
    wp, bqkv = attn_pack(a)
    xd, bq, bp, lw, lb = to_dev(dev, x, bqkv, a["bp"], a["lw"], a["lb"])
    wpd = wp.to(dev)
    out = Guarded(dev, (B, T, 120))
    rc = capi.load().d3il_attn_half_f16x3(xd.data_ptr(), lw.data_ptr(), lb.data_ptr(), float(a["eps"]), wpd.data_ptr(), bq.data_ptr(), bp.data_ptr(), out.ptr, B, T, 6, 120, stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and wpd is not None
    return out.read()


# ------------------------------------------------------------------------------------------------ 1. linear, shapes
@functools.lru_cache(maxsize=None)
def lin_weights(N):
    g = gen(300 + N)
    return torch.randn(N, 120, generator=g) * 0.09, torch.randn(N, generator=g) * 0.1


@functools.lru_cache(maxsize=None)
def lin_case(rows, N, form):
    """(x, W, bias, resid or None, ln or None, the f64 operand rows, want)."""
    eps, with_resid = LIN_FORMS[form]
    W, bias = lin_weights(N)
    g = gen(1000 + 7 * rows + N)
    x = torch.randn(rows, 120, generator=g) * 2 + 0.3 if eps else torch.randn(rows, 120, generator=g)
    ln = (1 + 0.3 * torch.randn(120, generator=g), 0.2 * torch.randn(120, generator=g), eps) if eps else None
    resid = torch.randn(rows, N, generator=g) * 1.5 if with_resid else None
    op = ln64(x, *ln) if ln else x.double()
    want = op @ W.double().t() + bias.double() + (resid.double() if with_resid else 0.0)
    return x, W, bias, resid, ln, op, want


def lin_yard(dev, x, W, bias, resid, ln):
    F = torch.nn.functional
    xd, Wd, bd, rd, lw, lb = to_dev(dev, x, W, bias, resid, *(ln[:2] if ln else (None, None)))
    y = F.linear(F.layer_norm(xd, (120,), lw, lb, ln[2]) if ln else xd, Wd, bd)
    return (y + rd if rd is not None else y).cpu()


@gpu
@pytest.mark.parametrize("form", list(LIN_FORMS))
@pytest.mark.parametrize("rows,N", LIN_PAIRS)
def test_linear_shapes_against_f64(dev, rows, N, form):
    x, W, bias, resid, ln, op, want = lin_case(rows, N, form)
    got = linear_launch(dev, x, W, bias, resid, ln)
    within("linear %dx%d %s" % (rows, N, form), got, want, lin_yard(dev, x, W, bias, resid, ln), 0 if ln else 1, floor_of(W, op))


# ------------------------------------------------------------------------------------------------ 2. linear, operand scale sweep
@functools.lru_cache(maxsize=None)
def sweep_case(which, e):
    """No LayerNorm, zero bias, no residual, N = 120, 33 rows: the rows (which = "x") or the weights ("w") times 2^e - exact scalings of one draw."""
    x, W = torch.randn(ROWS, 120, generator=gen(77)), torch.randn(120, 120, generator=gen(78)) * 0.09
    x, W = (x * 2.0 ** e, W) if which == "x" else (x, W * 2.0 ** e)
    return x, W, torch.zeros(120), x.double() @ W.double().t()


@gpu
@pytest.mark.parametrize("which,e", SWEEP)
def test_linear_operand_scale_sweep(dev, which, e):
    """The lower end of the operand range: at 2^-16 and 2^-20 the low halves (and at 2^-20 the high halves too) are subnormal f16 - matrix cores that flushed them
    would miss the bound grossly; the floor term is what the subnormal step itself costs."""
    x, W, bias, want = sweep_case(which, e)
    got = linear_launch(dev, x, W, bias)
    within("linear sweep %s 2^%d" % (which, e), got, want, lin_yard(dev, x, W, bias, None, None), 1, floor_of(W, x))


# ------------------------------------------------------------------------------------------------ 3. saturation values
@functools.lru_cache(maxsize=None)
def sat_case():
    W, bias = lin_weights(120)
    x = torch.randn(ROWS, 120, generator=gen(91))
    return x, W, bias


def sat_reference(dev, xc, W, bias):
    """(want, yardstick) of the rows xc, whose operands are finite and inside +-65504."""
    return xc.double() @ W.double().t() + bias.double(), lin_yard(dev, xc, W, bias, None, None)


@gpu
@pytest.mark.parametrize("k", range(len(SAT_VALUES) // len(SAT_ROWS)))
def test_linear_saturates_at_65504(dev, k):
    """One operand of a row in each of the three live waves replaced by a value at or beyond the f16 range: the row is that of the operand clamped to +-65504,
    every other row is bit-equal to the clean launch."""
    x, W, bias = sat_case()
    clean = linear_launch(dev, x, W, bias)
    vals = SAT_VALUES[3 * k:3 * k + 3]
    bad, clamped = x.clone(), x.clone()
    for r, c, v in zip(SAT_ROWS, SAT_COLS, vals):
        bad[r, c], clamped[r, c] = v, math.copysign(SAT, v)
    got = linear_launch(dev, bad, W, bias)
    keep = [r for r in range(ROWS) if r not in SAT_ROWS]
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    want, yard = sat_reference(dev, clamped, W, bias)
    for r, v in zip(SAT_ROWS, vals):
        assert bool(torch.isfinite(got[r]).all()), (r, v)
        within("linear saturation %g in row %d" % (v, r), got[r:r + 1], want[r:r + 1], yard[r:r + 1], 1, floor_of(W, clamped[r:r + 1]))


@gpu
def test_linear_nan_operand_saturates_to_one_bound(dev):
    """A NaN operand in a row of its own: the output is finite, it is the row of the operand := +65504 or := -65504 (printed), the same one on a second launch, and
    every other row is bit-equal to the clean launch.  Measured on the MI355X: -65504 (the clamp's maximum with -65504 comes first and returns its bound)."""
    x, W, bias = sat_case()
    clean = linear_launch(dev, x, W, bias)
    r, c = 20, 5
    bad = x.clone()
    bad[r, c] = float("nan")
    took = []
    for launch in range(2):
        got = linear_launch(dev, bad, W, bias)
        keep = [q for q in range(ROWS) if q != r]
        assert np.array_equal(bits(got[keep]), bits(clean[keep])) and bool(torch.isfinite(got[r]).all())
        fits = {}
        for sign in (1.0, -1.0):
            cl = x.clone()
            cl[r, c] = sign * SAT
            want, yard = sat_reference(dev, cl[r:r + 1], W, bias)
            err, ye, mag = float((got[r:r + 1].double() - want).abs().max()), float((yard.double() - want).abs().max()), float(want.abs().max())
            fits[sign] = (err, 4 * ye + 8 * U * mag + floor_of(W, cl[r:r + 1]))
            print("linear NaN operand, launch %d, against operand := %+g: kernel %.3e / bound %.3e" % (launch, sign * SAT, *fits[sign]))
        ok = [sign for sign, (err, bound) in fits.items() if err <= bound]
        assert len(ok) == 1, fits
        took.append(ok[0])
    print("linear NaN operand: taken as %+g" % (took[0] * SAT))
    assert took[0] == took[1]


# ------------------------------------------------------------------------------------------------ 4. MLP, shapes and gains
@functools.lru_cache(maxsize=None)
def mlp_net():
    g = gen(41)
    u = lambda *shape, fan: (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan)      # nn.Linear's initialisation
    return {"w1": u(480, 120, fan=120), "b1": u(480, fan=120), "w2": u(120, 480, fan=480), "b2": u(120, fan=480),
            "ln": (1 + 0.3 * torch.randn(120, generator=g), 0.2 * torch.randn(120, generator=g), 1e-5)}


def mlp_pre(h, with_ln, gain):
    """The f64 arguments of the GELU."""
    n = mlp_net()
    op = ln64(h, *n["ln"]) if with_ln else h.double()
    return op @ (n["w1"].double() * gain).t() + n["b1"].double()


def mlp_conditions(v, gain):
    """Per row of f64 pre-activations: arguments of erf inside (0.99, 1.01) - the seam of hx_erf2's two forms -; at gain 4 some beyond -5 and some beyond +5."""
    a = v.abs() / math.sqrt(2.0)
    seam, down, up = ((a > 0.99) & (a < 1.01)).sum(dim=1), (v < -5).sum(dim=1), (v > 5).sum(dim=1)
    return seam, down, up


@functools.lru_cache(maxsize=None)
def mlp_rows():
    """129 rows h and 129 other rows x.  Row 0 - the whole case at rows = 1 - is the first row of a pool that meets the conditions by itself in all four forms."""
    pool = torch.randn(2048, 120, generator=gen(43)) * 1.5 + 0.2
    ok = torch.ones(2048, dtype=torch.bool)
    for with_ln in (False, True):
        for gain in GAINS:
            seam, down, up = mlp_conditions(mlp_pre(pool, with_ln, gain), gain)
            ok &= (seam > 0) & ((down > 0) & (up > 0) if gain == 4 else torch.ones_like(ok))
    first = int(torch.nonzero(ok)[0])
    order = [first] + [i for i in range(max(MLP_ROWS) + 1) if i != first][:max(MLP_ROWS) - 1]
    return pool[order].contiguous(), torch.randn(max(MLP_ROWS), 120, generator=gen(44)) * 1.5


def mlp_want(h, x, with_ln, gain):
    n = mlp_net()
    return x.double() + torch.nn.functional.gelu(mlp_pre(h, with_ln, gain)) @ n["w2"].double().t() + n["b2"].double()


@gpu
@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("with_ln", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("same", [True, False], ids=["h_is_x", "h_not_x"])
@pytest.mark.parametrize("rows", MLP_ROWS)
def test_mlp_shapes_and_gains_against_f64(dev, rows, same, with_ln, gain):
    F = torch.nn.functional
    n, (H, X) = mlp_net(), mlp_rows()
    h, x = H[:rows].contiguous(), None if same else X[:rows].contiguous()
    ln = n["ln"] if with_ln else None
    want = mlp_want(h, h if same else x, with_ln, gain)
    hd, xd, w1, b1, w2, b2, lw, lb = to_dev(dev, h, h if same else x, n["w1"] * gain, n["b1"], n["w2"], n["b2"], n["ln"][0], n["ln"][1])
    yard = xd + F.linear(F.gelu(F.linear(F.layer_norm(hd, (120,), lw, lb, ln[2]) if ln else hd, w1, b1)), w2, b2)
    got = mlp_launch(dev, h, x, n["w1"] * gain, n["b1"], n["w2"], n["b2"], ln)
    within("mlp rows %d %s %s gain %d" % (rows, "h == x" if same else "h != x", "ln" if with_ln else "no ln", gain), got, want, yard, 1)


# ------------------------------------------------------------------------------------------------ 5. GELU seen through an identity MLP
def three_bits(c):
    m, e = math.frexp(c)
    return math.ldexp(round(m * 8) / 8, e)


@functools.lru_cache(maxsize=None)
def gelu_grid(i):
    """Band i: (h [129, 120] f32, b1 a scalar, v = h + b1 in f64).  h and b1 are multiples of delta = 2^(exponent of the largest magnitude around - 20): h has at
    most 21 significant bits (the split reproduces it), v at most 22 (the f32 sum is exact).  The band around 0 has b1 = 0 and +-0 among its points."""
    lo, hi = BANDS[i]
    b1 = 0.0 if lo < 0 < hi else three_bits(0.5 * (lo + hi))
    top = max(abs(lo), abs(hi), abs(lo - b1), abs(hi - b1))
    delta = 2.0 ** (math.floor(math.log2(top)) - 20)
    v = np.random.default_rng(900 + i).uniform(lo, hi, size=(GELU_ROWS, 120))
    h = np.round((v - b1) / delta) * delta
    h = np.where((h + b1 > lo) & (h + b1 < hi), h, np.round((0.5 * (lo + hi) - b1) / delta) * delta)
    if b1 == 0.0:
        h[0, 0], h[0, 1], h[GELU_ROWS - 1, 119], h[GELU_ROWS - 1, 118] = 0.0, -0.0, 0.0, -0.0
    return torch.from_numpy(h.astype(np.float32)), b1, torch.from_numpy(h + b1)


@functools.lru_cache(maxsize=None)
def identity_mlp(q):
    """fc1.weight[h, k] = [k == h mod 120], fc2.weight[c, h] = [h == c + 120 q]: out[r, c] = x[r, c] + b2[c] + GELU(h[r, c] + b1[c + 120 q])."""
    hid = torch.arange(480)
    w1, w2 = torch.zeros(480, 120), torch.zeros(120, 480)
    w1[hid, hid % 120] = 1.0
    w2[torch.arange(120), torch.arange(120) + 120 * q] = 1.0
    return w1, w2


@gpu
@pytest.mark.parametrize("q", range(4))
def test_gelu_bands_through_an_identity_mlp(dev, q):
    """out = GELU(v) with nothing else in the way, band by band; the other three quarters of the hidden layer carry another bias (b1 + 3.25, + 6.5, ..: a GELU value
    from a neighbouring hidden pair or bias row would be off by far more than any bound), so each of the 120 columns also checks that stage k pairs the first
    product of hidden pair k - 1 with ITS bias row and ITS second-product weights, the two empty half stages included."""
    w1, w2 = identity_mlp(q)
    zeros = torch.zeros(GELU_ROWS, 120)
    for i, band in enumerate(BANDS):
        h, b1, v = gelu_grid(i)
        b1v = torch.cat([torch.full((120,), b1 + 3.25 * ((j - q) % 4)) for j in range(4)])
        got = mlp_launch(dev, h, zeros, w1, b1v, w2, torch.zeros(120))
        yard = torch.nn.functional.gelu(v.to(torch.float32).to(dev))
        within("gelu quarter %d band (%g, %g)" % (q, *band), got, torch.nn.functional.gelu(v), yard, 1)


# ------------------------------------------------------------------------------------------------ 6. attention half
@functools.lru_cache(maxsize=None)
def attn_params(kind):
    g = gen(61)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(120)
    a = {k: u(120, 120) for k in ("wq", "wk", "wv", "wp")}
    a.update({k: u(120) for k in ("bq", "bk", "bv", "bp")})
    a.update(lw=1 + 0.3 * torch.randn(120, generator=g), lb=0.2 * torch.randn(120, generator=g), eps=1e-5)
    for k in ("wq", "wk", "bq", "bk"):
        a[k] = a[k] * ATT_SCALE[kind]
    return a


def attn_half(a, x, dev=None):
    """x + proj(causal_softmax_attention(ln1(x) Wqkv + b)) + bproj in the dtype of x (f64 on the CPU: the reference; f32 on `dev`: torch's layers, the yardstick):
    (output, scores [B, 6, T, T] with -inf above the diagonal)."""
    F = torch.nn.functional
    B, T, _ = x.shape
    p = {k: (v.to(x.dtype) if dev is None else v.to(dev)) for k, v in a.items() if torch.is_tensor(v)}
    xx = x if dev is None else x.to(dev)
    op = ln64(xx, p["lw"], p["lb"], a["eps"]) if dev is None else F.layer_norm(xx, (120,), p["lw"], p["lb"], a["eps"])
    qkv = F.linear(op, torch.cat((p["wq"], p["wk"], p["wv"]), 0), torch.cat((p["bq"], p["bk"], p["bv"]), 0))
    y, scores = f32e.attention(qkv, B, T, 6, 20)
    return xx + F.linear(y, p["wp"], p["bp"]), scores


@functools.lru_cache(maxsize=None)
def attn_case(B, T, kind):
    x = torch.randn(B, T, 120, generator=gen(5000 + 100 * B + T)) * 1.5 + 0.2
    want, scores = attn_half(attn_params(kind), x.double())
    return x, want, scores


@gpu
@pytest.mark.parametrize("kind", list(ATT_SCALE))
@pytest.mark.parametrize("B,T", ATT_CASES)
def test_attention_half_against_f64(dev, B, T, kind):
    a = attn_params(kind)
    x, want, _ = attn_case(B, T, kind)
    yard = attn_half(a, x, dev)[0].cpu()
    within("attention half B %d T %d %s" % (B, T, kind), attn_launch(dev, a, x), want, yard, 1)


@gpu
def test_attention_token_0_sees_no_other_token(dev):
    """sharp, T = 11: the row of token 0 of every sequence is bit-equal when tokens 1 .. 10 are replaced by other finite values."""
    a = attn_params("sharp")
    x = attn_case(9, 11, "sharp")[0]
    other = x.clone()
    other[:, 1:] = torch.randn(9, 10, 120, generator=gen(62)) * 3 - 0.5
    one, two = attn_launch(dev, a, x), attn_launch(dev, a, other)
    assert np.array_equal(bits(one[:, 0].contiguous()), bits(two[:, 0].contiguous()))
    assert not np.array_equal(bits(one[:, 1:].contiguous()), bits(two[:, 1:].contiguous()))


# ------------------------------------------------------------------------------------------------ 7. non-finite operands in the default instantiations
NF_NAN, NF_INF = 9, NF_ROWS - 1      # row 9 shares its tile with clean rows; row 36 is the one the dead lanes re-read


def show(tag, rows):
    print("%s: %s" % (tag, "; ".join("finite %d of %d, first values %s" % (int(torch.isfinite(r).sum()), r.numel(), r.reshape(-1)[:4].tolist()) for r in rows)))


@gpu
@pytest.mark.parametrize("N", [360, 120])
def test_linear_nonfinite_rows_stay_alone(dev, N):
    """A NaN operand in row 9, +Inf in row 36: every other row is bit-equal to the clean launch; the hit rows are what two launches agree on (printed)."""
    W, bias = lin_weights(N)
    x = torch.randn(NF_ROWS, 120, generator=gen(71))
    clean = linear_launch(dev, x, W, bias)
    bad = x.clone()
    bad[NF_NAN, 3], bad[NF_INF, 119] = float("nan"), float("inf")
    one, two = linear_launch(dev, bad, W, bias), linear_launch(dev, bad, W, bias)
    keep = [r for r in range(NF_ROWS) if r not in (NF_NAN, NF_INF)]
    assert np.array_equal(bits(one[keep]), bits(clean[keep])) and np.array_equal(bits(one), bits(two))
    show("unguarded linear N = %d, NaN row / Inf row" % N, (one[NF_NAN], one[NF_INF]))


@gpu
@pytest.mark.parametrize("with_ln", [True, False], ids=["ln", "noln"])
def test_mlp_nonfinite_rows_stay_alone(dev, with_ln):
    n = mlp_net()
    x = torch.randn(NF_ROWS, 120, generator=gen(72))
    args = (n["w1"], n["b1"], n["w2"], n["b2"], n["ln"] if with_ln else None)
    clean = mlp_launch(dev, x, None, *args)
    bad = x.clone()
    bad[NF_NAN, 3], bad[NF_INF, 119] = float("nan"), float("inf")
    one, two = mlp_launch(dev, bad, None, *args), mlp_launch(dev, bad, None, *args)
    keep = [r for r in range(NF_ROWS) if r not in (NF_NAN, NF_INF)]
    assert np.array_equal(bits(one[keep]), bits(clean[keep])) and np.array_equal(bits(one), bits(two))
    show("unguarded mlp %s, NaN row / Inf row" % ("ln" if with_ln else "no ln"), (one[NF_NAN], one[NF_INF]))


@gpu
@pytest.mark.parametrize("B,T", NF_ATT)
def test_attention_nonfinite_tokens_reach_only_their_own_later_tokens(dev, B, T):
    """NaN in token 4 of sequence 1, +Inf in token 7 of sequence 2: sequence 0 (and 3, 4), and the tokens in front of the hit token in its own sequence, are
    bit-equal to the clean launch; the rest of the two sequences is what two launches agree on (printed)."""
    a = attn_params("randn")
    x = torch.randn(B, T, 120, generator=gen(73 + T))
    clean = attn_launch(dev, a, x)
    bad = x.clone()
    bad[1, 4, 0], bad[2, 7, 119] = float("nan"), float("inf")
    one, two = attn_launch(dev, a, bad), attn_launch(dev, a, bad)
    same = torch.ones(B, T, dtype=torch.bool)
    same[1, 4:], same[2, 7:] = False, False
    assert np.array_equal(bits(one[same]), bits(clean[same])) and np.array_equal(bits(one), bits(two))
    show("unguarded attention half B %d T %d, NaN token and the next / Inf token and the next" % (B, T), (one[1, 4], one[1, 5], one[2, 7], one[2, 8]))


# ------------------------------------------------------------------------------------------------ 8. refusals before any launch
def untouched(g):
    return bool((g.bits() == SENT.view(np.uint32)).all())


@gpu
def test_linear_entry_refuses_before_any_launch(dev):
    from d3il_amd import capi
    L = capi.load()
    rows, N = 5, 120
    W, bias = lin_weights(N)
    x, resid, lw, lb = (torch.randn(*s, generator=gen(81)) for s in ((rows, 120), (rows, N), (120,), (120,)))
    xd, bd, rd, lwd, lbd = to_dev(dev, x, bias, resid, lw, lb)
    from d3il_amd import policies as P
    wp = P.pack_linear120_weights_f16x3(W).to(dev)
    base = dict(xin=xd.data_ptr(), lw=lwd.data_ptr(), lb=lbd.data_ptr(), wp=wp.data_ptr(), bias=bd.data_ptr(), resid=rd.data_ptr(), rows=rows, N=N, shift=0)

    def call(**kw):
        a = dict(base, **kw)
        out = Guarded(dev, (max(a["rows"], 1), 388), a["shift"])
        rc = L.d3il_linear120_f16x3(a["xin"], a["lw"], a["lb"], 1e-5, a["wp"], a["bias"], a["resid"], out.ptr, a["rows"], a["N"], stream(dev))
        torch.cuda.synchronize(dev)
        return rc, untouched(out)

    keep = []
    for name, t in (("xin", x), ("bias", bias), ("resid", resid)):
        k, p = shifted(dev, t, 1)
        keep.append(k)
        assert call(**{name: p}) == (EINVAL, True), name
    k, p = shifted(dev, wp.view(torch.float32), 1)
    assert call(wp=p) == (EINVAL, True) and call(shift=1) == (EINVAL, True) and k is not None
    for n in (0, 2, 6, 388):
        assert call(N=n) == (EINVAL, True), n
    assert call(lb=None) == (EINVAL, True) and call(lw=None) == (EINVAL, True)
    assert call(rows=-1) == (EINVAL, True)
    assert call(rows=0) == (0, True)
    assert call(lw=None, lb=None, resid=None)[0] == 0


@gpu
def test_mlp_entry_refuses_before_any_launch(dev):
    """b1 among the pointers: k_mlp_gelu_residual_f16x3 copies fc1's bias to LDS with 16-byte loads (the f32 kernel reads it by scalars, its entry does not ask)."""
    from d3il_amd import capi, policies as P
    L = capi.load()
    n, rows = mlp_net(), 5
    h, x = torch.randn(rows, 120, generator=gen(82)), torch.randn(rows, 120, generator=gen(83))
    hd, xd, b1d, b2d, lwd, lbd = to_dev(dev, h, x, n["b1"], n["b2"], n["ln"][0], n["ln"][1])
    wp = P.pack_mlp_weights_f16x3(n["w1"], n["w2"]).to(dev)
    base = dict(h=hd.data_ptr(), lw=lwd.data_ptr(), lb=lbd.data_ptr(), x=xd.data_ptr(), wp=wp.data_ptr(), b1=b1d.data_ptr(), b2=b2d.data_ptr(), rows=rows, C=120, H=480, shift=0)

    def call(**kw):
        a = dict(base, **kw)
        out = Guarded(dev, (max(a["rows"], 1), 120), a["shift"])
        rc = L.d3il_mlp_ln_gelu_residual_f16x3(a["h"], a["lw"], a["lb"], 1e-5, a["x"], a["wp"], a["b1"], a["b2"], out.ptr, a["rows"], a["C"], a["H"], stream(dev))
        torch.cuda.synchronize(dev)
        return rc, untouched(out)

    keep = []
    for name, t in (("h", h), ("x", x), ("b1", n["b1"]), ("b2", n["b2"])):
        k, p = shifted(dev, t, 1)
        keep.append(k)
        assert call(**{name: p}) == (EINVAL, True), name
    k, p = shifted(dev, wp.view(torch.float32), 1)
    assert call(wp=p) == (EINVAL, True) and call(shift=1) == (EINVAL, True) and k is not None
    assert call(C=124) == (EUNSUPPORTED, True) and call(C=116) == (EUNSUPPORTED, True) and call(H=512) == (EUNSUPPORTED, True)
    assert call(lb=None) == (EINVAL, True) and call(lw=None) == (EINVAL, True)
    assert call(rows=-1) == (EINVAL, True)
    assert call(rows=0) == (0, True)
    assert call(lw=None, lb=None)[0] == 0 and call()[0] == 0


@gpu
def test_attention_entry_refuses_before_any_launch(dev):
    from d3il_amd import capi
    L = capi.load()
    a, B, T = attn_params("randn"), 3, 11
    wp, bqkv = attn_pack(a)
    x = torch.randn(B, T, 120, generator=gen(84))
    xd, bq, bp, lwd, lbd = to_dev(dev, x, bqkv, a["bp"], a["lw"], a["lb"])
    wpd = wp.to(dev)
    base = dict(x=xd.data_ptr(), lw=lwd.data_ptr(), lb=lbd.data_ptr(), wp=wpd.data_ptr(), bq=bq.data_ptr(), bp=bp.data_ptr(), B=B, T=T, nh=6, C=120, shift=0, out=None)

    def call(**kw):
        c = dict(base, **kw)
        out = Guarded(dev, (max(c["B"], 1), 17, 124), c["shift"])
        rc = L.d3il_attn_half_f16x3(c["x"], c["lw"], c["lb"], 1e-5, c["wp"], c["bq"], c["bp"], c["out"] or out.ptr, c["B"], c["T"], c["nh"], c["C"], stream(dev))
        torch.cuda.synchronize(dev)
        return rc, untouched(out)

    keep = []
    for name, t in (("x", x), ("bq", bqkv), ("bp", a["bp"]), ("lw", a["lw"]), ("lb", a["lb"])):
        k, p = shifted(dev, t, 1)
        keep.append(k)
        assert call(**{name: p}) == (EINVAL, True), name
    k, p = shifted(dev, wpd.view(torch.float32), 1)
    assert call(wp=p) == (EINVAL, True) and call(shift=1) == (EINVAL, True) and k is not None
    for t in (0, 17):
        assert call(T=t) == (EINVAL, True), t
    assert call(nh=5) == (EUNSUPPORTED, True) and call(nh=4) == (EUNSUPPORTED, True)
    assert call(C=124) == (EUNSUPPORTED, True) and call(C=100) == (EUNSUPPORTED, True)
    before = xd.clone()
    assert call(out=xd.data_ptr()) == (EINVAL, True) and torch.equal(xd, before)      # out == x
    assert call(lb=None) == (EINVAL, True) and call(lw=None) == (EINVAL, True)
    assert call(B=-1) == (EINVAL, True)
    assert call(B=0) == (0, True)
    assert call()[0] == 0


# ------------------------------------------------------------------------------------------------ 9. the inputs do their job (no GPU)
def test_the_inputs_do_their_job():
    """On the f64 references and the host's split alone: the sweep's top scale stays inside +-65504 and its bottom scales reach subnormal f16 halves; the saturation
    rows sit in three waves, the last live row among them; every MLP case has erf arguments on the seam of hx_erf2 and, at gain 4, pre-activations beyond +-5; the
    GELU grids are reproduced by the split, their bias sum is exact in f32, every band holds its 15480 points; the attention regimes are sharp and flat."""
    from d3il_amd.policies import split_f16
    # 1: every row count and every N in every form
    assert {r for r, _ in LIN_PAIRS} == set(LIN_ROWS) and {n for _, n in LIN_PAIRS} == set(LIN_N)
    for form in LIN_FORMS:
        ln = lin_case(17, 20, form)[4]
        assert ln is None or (float((ln[0] - 1).abs().max()) > 0.3 and float(ln[1].abs().max()) > 0.2)
    # 2: the sweep
    for which, e in SWEEP:
        x, W, _, want = sweep_case(which, e)
        t = x if which == "x" else W
        hi, lo = split_f16(t)
        sub_hi, sub_lo = int(((hi != 0) & (hi.abs().float() < 2.0 ** -14)).sum()), int(((lo != 0) & (lo.abs().float() < 2.0 ** -14)).sum())
        print("sweep %s 2^%d: max |operand| %.4g, subnormal high halves %d, subnormal low halves %d of %d, max |want| %.3g" % (which, e, float(t.abs().max()), sub_hi, sub_lo, t.numel(), float(want.abs().max())))
        assert float(x.abs().max()) < SAT and float(W.abs().max()) < SAT
        if e <= -16:
            assert sub_lo > t.numel() // 2
        if e == -20:
            assert sub_hi > t.numel() // 2
        if e >= 0:
            assert sub_lo < t.numel() // 8
    assert float(sweep_case("x", 14)[0].abs().max()) > SAT / 2
    # 3: three waves, the last live row
    assert sorted(r // 16 for r in SAT_ROWS) == [0, 1, 2] and ROWS - 1 in SAT_ROWS and len(SAT_VALUES) % len(SAT_ROWS) == 0
    assert float(sat_case()[0].abs().max()) < 6
    # 4: the MLP cases
    H, _ = mlp_rows()
    for rows in MLP_ROWS:
        for with_ln in (True, False):
            for gain in GAINS:
                v = mlp_pre(H[:rows], with_ln, gain)
                seam, down, up = (int(c.sum()) for c in mlp_conditions(v, gain))
                print("mlp rows %d %s gain %d: erf arguments inside (0.99, 1.01): %d, pre-activations < -5: %d, > 5: %d, max |v| %.2f" % (rows, "ln" if with_ln else "no ln", gain, seam, down, up, float(v.abs().max())))
                assert seam > 0 and (gain == 1 or (down > 0 and up > 0)), (rows, with_ln, gain)
    # 5: the GELU grids
    for i, (lo, hi) in enumerate(BANDS):
        h, b1, v = gelu_grid(i)
        sh, sl = split_f16(h)
        assert torch.equal(sh.double() + sl.double() / 2048.0, h.double()), (lo, hi)                         # the split reproduces h
        assert float(np.float32(b1)) == b1 and torch.equal((h + torch.tensor(b1, dtype=torch.float32)).double(), v), (lo, hi)      # the f32 sum h + b1 is exact
        assert bool(((v > lo) & (v < hi)).all()) and v.numel() == GELU_ROWS * 120 and len(np.unique(v.numpy())) > 300, (lo, hi)
        assert float(v.min()) < lo + 0.05 * (hi - lo) and float(v.max()) > hi - 0.05 * (hi - lo)
        if lo < 0 < hi:
            z = h.numpy().reshape(-1)
            assert b1 == 0.0 and int(((z == 0) & ~np.signbit(z)).sum()) >= 2 and int(((z == 0) & np.signbit(z)).sum()) >= 2
    for q in range(4):
        w1, w2 = identity_mlp(q)
        assert float(w1.sum()) == 480 and float(w2.sum()) == 120 and bool((w1.sum(dim=1) == 1).all()) and bool((w2.sum(dim=1) == 1).all())
    # 6: the attention regimes
    for B, T in ATT_CASES:
        valid = torch.tril(torch.ones(T, T)) > 0
        std = {kind: float(attn_case(B, T, kind)[2][..., valid].std(unbiased=False)) for kind in ATT_SCALE}
        print("attention B %d T %d: standard deviation of the f64 scores: %s" % (B, T, ", ".join("%s %.3g" % kv for kv in std.items())))
        assert std["sharp"] >= 30 and std["flat"] <= 1e-3 and 0.1 < std["randn"] < 3, (B, T, std)
    assert all(B == (9 if T <= 11 else 5) for B, T in ATT_CASES[:16]) and [T for _, T in ATT_CASES[:16]] == list(range(1, 17)) and ATT_CASES[16:] == [(1, 11), (1, 16)]
