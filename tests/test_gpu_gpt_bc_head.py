"""d3il_gpt_bc_head_f32 (csrc/policy_gpt_bc.h) on the GPU against an f64 torch restatement: 257 rows = 64 full waves' worth of four-row workgroups and a tail of one;
launches of 1, 63, 64, 65 and 257 rows, C in {72, 120} (the reference's widths: one and two elements per lane), A in {2, 3, 8}.  The yardstick of every accuracy
assertion is the deviation of torch's own f32 LayerNorm and head on the same rows and device from the f64 result, measured here and printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 257
ROWS = (1, 63, 64, 65, 257)
CASES = [(C, A) for C in (72, 120) for A in (2, 3, 8)]
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class Case:
    """LayerNorm parameters, head rows, bounds (+-1.2 against outputs of about one: some reach the clamp), scale and shift, hidden rows - and, computed once, the
    f64 result on the host and torch's f32 result on the device."""

    def __init__(self, C, A, dev):
        g = torch.Generator().manual_seed(100 * C + A)
        self.C, self.A = C, A
        self.ln_w, self.ln_b = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        self.w = torch.randn(A, C, generator=g) / C ** 0.5
        self.lo, self.hi = -1.2 - 0.1 * torch.rand(A, generator=g), 1.2 + 0.1 * torch.rand(A, generator=g)
        self.scale, self.shift = 0.004 + 0.001 * torch.rand(A, generator=g), 0.001 * torch.arange(A, dtype=torch.float32) - 0.003
        self.h = torch.randn(N, C, generator=g) * 1.5 + 0.3
        self.eps = 1e-5
        self.want, self.raw = self.torch_tail(self.h.double(), torch.float64, "cpu")
        self.t32 = self.torch_tail(self.h.to(dev), torch.float32, dev)[0].cpu()
        self.yard = float((self.t32.double() - self.want).abs().max())
        self.on = tuple(v.to(dev).contiguous() for v in (self.ln_w, self.ln_b, self.w, self.lo, self.hi, self.scale, self.shift))

    def torch_tail(self, h, dt, dev):
        f = lambda v: v.to(device=dev, dtype=dt)
        x = torch.nn.functional.layer_norm(h, (self.C,), f(self.ln_w), f(self.ln_b), self.eps)
        o = torch.nn.functional.linear(x, f(self.w))
        y = (torch.minimum(torch.maximum(o, f(self.lo)), f(self.hi)).double() * self.scale.to(dev).double() + self.shift.to(dev).double()).to(dt)
        return y, o


def case(C, A, dev):
    if (C, A) not in _CACHE:
        _CACHE[(C, A)] = Case(C, A, dev)
    return _CACHE[(C, A)]


class Launch:
    """One call of the entry point; the outputs are poisoned with 777 before the call."""

    def __init__(self, dev, c, n=N, first=0, h=None, bad=True, **over):
        from d3il_amd import capi
        ht = (c.h if h is None else h)[first:first + n].to(dev).contiguous()
        C_, A_ = over.get("C", c.C), over.get("A", c.A)
        ln_w, ln_b, w, lo, hi, sc, sh = c.on
        act = torch.full((n, max(c.A, A_, 1)), 777.0, device=dev)
        flag = torch.full((n,), 777, dtype=torch.int32, device=dev)
        self.rc = capi.load().d3il_gpt_bc_head_f32(ht.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), c.eps, w.data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                                   act.data_ptr(), flag.data_ptr() if bad else None, n, C_, A_, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        self.keep = ht
        self.poison = act.cpu()
        self.actions, self.bad = act[:, :c.A].cpu().contiguous(), flag.cpu()

    def bits(self):
        return self.actions.numpy().view(np.uint32)


@pytest.mark.parametrize("C,A", CASES)
def test_actions_against_f64(dev, C, A):
    c = case(C, A, dev)
    whole = Launch(dev, c)
    assert whole.rc == 0 and not bool(whole.bad.any())
    clamped = int(((c.raw < c.lo.double()) | (c.raw > c.hi.double())).sum())
    assert 0 < clamped < c.raw.numel()      # both sides of the clamp
    err = float((whole.actions.double() - c.want).abs().max())
    print("C %d A %d: kernel %.3e, torch f32 %.3e -> %.2f yardsticks (%d of %d outputs clamped)" % (C, A, err, c.yard, err / c.yard, clamped, c.raw.numel()))
    assert c.yard > 0 and err <= 4 * c.yard
    # every row count: the rows of a smaller launch - and of a launch that starts elsewhere - are the rows of the whole one, bit for bit
    for n in ROWS[:-1]:
        part = Launch(dev, c, n=n)
        assert part.rc == 0 and np.array_equal(part.bits(), whole.bits()[:n]), n
    assert np.array_equal(Launch(dev, c, n=70, first=130).bits(), whole.bits()[130:200])
    assert np.array_equal(Launch(dev, c, bad=False).bits(), whole.bits())      # without the flags: the same actions


def test_clamp_edges_are_exact(dev):
    """Outputs driven past both bounds come out as inverse_scale(bound) bit for bit: f64 product and sum of the f32 operands, rounded once."""
    c = case(120, 8, dev)
    big = Case(120, 8, dev)
    big.w = c.w * 1e3
    big.on = tuple(v.to(dev).contiguous() for v in (big.ln_w, big.ln_b, big.w, big.lo, big.hi, big.scale, big.shift))
    out = Launch(dev, big)
    raw = big.torch_tail(big.h.double(), torch.float64, "cpu")[1]
    far = (raw > 5) | (raw < -5)      # (an output of the scaled head that still lies inside the bounds is not an edge)
    assert float(far.float().mean()) > 0.98
    want_hi = (big.hi.double() * big.scale.double() + big.shift.double()).float()
    want_lo = (big.lo.double() * big.scale.double() + big.shift.double()).float()
    want = torch.where(raw > 0, want_hi.expand(N, 8), want_lo.expand(N, 8))
    assert np.array_equal(out.bits()[far.numpy()], want.contiguous().numpy().view(np.uint32)[far.numpy()])


@pytest.mark.parametrize("C,A", [(72, 2), (120, 8)])
def test_nonfinite_rows_are_marked_alone(dev, C, A):
    c = case(C, A, dev)
    clean = Launch(dev, c)
    h = c.h.clone()
    h[3, C - 1], h[64, 0], h[200, 70], h[256, 1] = float("nan"), float("inf"), float("-inf"), float("nan")      # (256: the tail row)
    h[100] = 3e38      # finite, but the row's variance leaves the f32 range
    out = Launch(dev, c, h=h)
    hit = [3, 64, 100, 200, 256]
    good = [r for r in range(N) if r not in hit]
    assert np.array_equal(out.bits()[hit], np.full((5, A), 0x7FC00000, dtype=np.uint32))
    assert out.bad[hit].tolist() == [1] * 5 and not bool(out.bad[good].any())
    assert np.array_equal(out.bits()[good], clean.bits()[good])


def test_unsupported_shapes_are_refused_before_any_launch(dev):
    from d3il_amd import capi
    c = case(120, 8, dev)
    for kw in (dict(C=132), dict(C=0), dict(C=70), dict(A=17), dict(A=0)):
        o = Launch(dev, c, n=4, **kw)
        assert o.rc == -5, kw
        assert bool((o.poison == 777.0).all()) and bool((o.bad == 777).all()), kw
    assert b"d3il_gpt_bc_head_f32" in capi.load().d3il_last_error()
    ok = Launch(dev, c, n=4)
    assert ok.rc == 0 and torch.isfinite(ok.actions).all() and not bool((ok.actions == 777.0).any())
    ln_w, ln_b, w, lo, hi, sc, sh = c.on
    act = torch.full((4, 8), 777.0, device=dev)
    lib = capi.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert lib.d3il_gpt_bc_head_f32(None, ln_w.data_ptr(), ln_b.data_ptr(), c.eps, w.data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(), sh.data_ptr(), act.data_ptr(), None, 4, 120, 8, stream) == -1
    assert lib.d3il_gpt_bc_head_f32(ok.keep.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), c.eps, w.data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(), sh.data_ptr(), None, None, 4, 120, 8, stream) == -1
    assert lib.d3il_gpt_bc_head_f32(ok.keep.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), c.eps, w.data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(), sh.data_ptr(), act.data_ptr(), None, -1, 120, 8, stream) == -1
    assert lib.d3il_gpt_bc_head_f32(ok.keep.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), c.eps, w.data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(), sh.data_ptr(), act.data_ptr(), None, 0, 120, 8, stream) == 0
    torch.cuda.synchronize()
    assert bool((act == 777.0).all())
