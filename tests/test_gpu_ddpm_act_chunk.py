"""k_ddpm_act_chunk (csrc/policy_ddpm_act.h) through d3il_ddpm_act_chunk_f32 on the GPU against an f64 NumPy restatement written out here (``np_eps`` / ``np_step``:
DiffusionEncDec.forward and one reverse step of Diffusion.sample on the state dict alone), all banks given unless the test is about Philox.

Geometry: one workgroup of four waves per 16 environments; 17 environments = one full tile and a tail tile of one.  Shapes (obs, A, obs_seq_len S, action_seq_len
Ta, encoder layers, decoder layers, timesteps T): (4, 2, 1, 1, 1, 1, 2) - one state token, one action token -, (10, 2, 5, 4, 2, 4, 16) - the shipped one - and
(32, 8, 5, 4, 2, 4, 4) - two full input tiles, both action lane groups; window lengths ragged over 1 .. S.  The yardstick of a case is the deviation of torch's own
f32 evaluation of that case (policies.DDPMACTPolicy._chain_torch, its own layers, on the same device) from the f64 restatement, taken per case and never carried
over; the bar is 4 of them plus 4 x 2^-24 x max |want|.  Every output sits inside a larger buffer with 64 sentinel words in front and behind."""
import functools
import math
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 17
CASES = {"tiny": (4, 2, 1, 1, 1, 1, 2), "shipped": (10, 2, 5, 4, 2, 4, 16), "wide": (32, 8, 5, 4, 2, 4, 4)}
POISON, GUARD = 777.0, 64
EUNSUPPORTED = -5
_erf = np.vectorize(math.erf)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- the f64 NumPy restatement (one environment at a time: its own window length)
def np_eps(sd, x, i, st, heads=4):
    """eps [Ta, A] of DiffusionEncDec.forward for the iterate x [Ta, A], chain step i and the window st [L, obs]."""
    C = sd["tok_emb.weight"].shape[0]
    hd = C // heads
    lin = lambda v, p: v @ sd[p + ".weight"].T + sd[p + ".bias"]

    def ln(v, p):
        m = v.mean(axis=-1, keepdims=True)
        return (v - m) / np.sqrt(((v - m) ** 2).mean(axis=-1, keepdims=True) + 1e-5) * sd[p + ".weight"]

    def attend(q, k, v, causal):
        out = np.zeros_like(q)
        for h in range(heads):
            sl = slice(h * hd, (h + 1) * hd)
            s = q[:, sl] @ k[:, sl].T / math.sqrt(hd)
            if causal:
                s = np.where(np.tril(np.ones(s.shape)) > 0, s, -np.inf)
            p = np.exp(s - s.max(axis=-1, keepdims=True))
            out[:, sl] = (p / p.sum(axis=-1, keepdims=True)) @ v[:, sl]
        return out

    def stack(v, name, cond):
        l = 0
        while "%s.blocks.%d.ln1.weight" % (name, l) in sd:
            p = "%s.blocks.%d." % (name, l)
            h = ln(v, p + "ln1")
            y = attend(lin(h, p + "attn.query"), lin(h, p + "attn.key"), lin(h, p + "attn.value"), True)
            if cond is not None:
                y = y + attend(lin(h, p + "attn.cross_query"), lin(cond, p + "attn.cross_key"), lin(cond, p + "attn.cross_value"), False)
            v = v + lin(y, p + "attn.proj")
            u = lin(ln(v, p + "ln2"), p + "mlp.0")
            v = v + lin(0.5 * u * (1.0 + _erf(u / math.sqrt(2.0))), p + "mlp.2")
            l += 1
        return ln(v, name + ".ln")

    L, Ta = st.shape[0], x.shape[0]
    half = C // 2
    e = float(i) * np.exp(np.arange(half) * -(math.log(10000) / (half - 1)))
    u = lin(np.concatenate((np.sin(e), np.cos(e)))[None, :], "time_emb.1")
    te = lin(u * np.tanh(np.log1p(np.exp(u))), "time_emb.3")      # Mish
    pos = sd["pos_emb"][0]
    enc = stack(np.concatenate([te, lin(st, "tok_emb") + pos[:L]], axis=0), "encoder", None)
    return lin(stack(lin(x, "action_emb") + pos[L - 1:L - 1 + Ta], "decoder", enc), "action_pred")


def np_step(c, x, i, st, noise):
    """One reverse step of Diffusion.sample in f64 on the f32 schedule table's f64 twin."""
    s = c.sched64[i]
    x0 = np.clip(s[0] * x - s[1] * np_eps(c.sd, x, i, st), c.lo64, c.hi64)
    mean = s[2] * x0 + s[3] * x
    return mean if i == 0 else mean + s[4] * noise


@functools.lru_cache(maxsize=None)
def case(name):
    """Network, inputs and the shared f64 references of a case (computed once, shared, never modified)."""
    from d3il_amd import policies as P
    obs, A, S, Ta, enc, dec, T = CASES[name]
    pol = P.DDPMACTPolicy.random(obs, A, device="cpu", seed=11, obs_seq_len=S, action_seq_len=Ta, n_timesteps=T, enc_layers=enc, dec_layers=dec, policy_seed=23, bound=2.5)
    g = torch.Generator().manual_seed(7)
    win = torch.randn(N, S, obs, generator=g) * 0.7
    ln = torch.tensor([1 + (i * 3) % S for i in range(N)], dtype=torch.int64)      # ragged: 1, 4, 2, 5, 3, ..
    for i in range(N):
        win[i, int(ln[i]):] = 0.0      # the padded() form: zeros behind the valid rows
    noise = torch.randn(N, T + 1, Ta, A, generator=g)
    x_in = torch.randn(N, Ta, A, generator=g) * 1.2
    prior = torch.randn(N, Ta, A, generator=g) * 0.002      # what the lanes that are not due emit from
    sd = {k: v.double().numpy() for k, v in pol.model.state_dict().items()}
    c = types.SimpleNamespace(name=name, obs=obs, A=A, S=S, Ta=Ta, enc=enc, dec=dec, T=T, pol=pol, win=win, len=ln, noise=noise, x_in=x_in, prior=prior, sd=sd, pk=pol._pack(),
                              sched64=P.ddpm_schedule(P.cosine_beta_schedule(T).double())["sched"].numpy(), lo64=pol.lo.double().numpy(), hi64=pol.hi.double().numpy())
    return c


@functools.lru_cache(maxsize=None)
def step_ref(name, k):
    """The f64 result of chain step k from x_in for every environment of a case: [N, Ta, A]."""
    c = case(name)
    return np.stack([np_step(c, c.x_in[i].double().numpy(), k, c.win[i, :int(c.len[i])].double().numpy(), c.noise[i, k].double().numpy()) for i in range(N)])


def torch_f32(dev, c, x=None, k_start=None, k_stop=0):
    """torch's own f32 evaluation on the device, lanes grouped by window length: (chunk, last iterate)."""
    import copy
    p32 = copy.copy(c.pol)
    p32.model = copy.deepcopy(c.pol.model).to(dev)
    p32._sched = c.pol._sched.to(dev)
    for k in ("lo", "hi", "out_scale", "out_shift"):
        setattr(p32, k, getattr(c.pol, k).to(dev))
    chunk, last = torch.zeros(N, c.Ta, c.A), torch.zeros(N, c.Ta, c.A)
    for L in sorted(set(c.len.tolist())):
        sel = torch.nonzero(c.len == L).reshape(-1)
        y, _, xl = p32._chain_torch(c.win[sel, :L].to(dev), c.noise[sel].to(dev), x=None if x is None else x[sel].to(dev), k_start=k_start, k_stop=k_stop)
        chunk[sel], last[sel] = y.cpu(), xl.cpu()
    return chunk, last


def guarded(dev, shape, dtype, fill):
    """A buffer of ``shape`` inside a flat one with GUARD sentinel words in front and behind: (flat, view)."""
    size = int(np.prod(shape))
    flat = torch.full((size + 2 * GUARD,), 12345 if dtype == torch.int32 else 4242.0, dtype=dtype, device=dev)
    view = flat[GUARD:GUARD + size].view(*shape)
    if torch.is_tensor(fill):
        view.copy_(fill.to(device=dev, dtype=dtype))
    else:
        view.fill_(fill)
    return flat, view


class Launch:
    """One call of the entry point on rows of a case.  ``counter`` / ``chunk``: the persistent state before the call (default: every lane due, chunk poisoned);
    ``noise``: "bank" (the case's), None (Philox) or a tensor; ``x``: None, "bank" (the case's x_in) or a tensor."""

    def __init__(self, dev, c, n=N, win=None, ln=None, noise="bank", x=None, k_start=-1, k_stop=0, counter=None, chunk=None, env_offset=0, seed=23, t=0, rows=None, **over):
        from d3il_amd import capi
        rows = slice(0, n) if rows is None else rows
        f = lambda v: v.to(dev).contiguous()
        pk = {k: f(v) for k, v in c.pk.items()}
        pol = c.pol
        wn = f((c.win if win is None else win)[rows].clone())
        lens = f((c.len if ln is None else ln)[rows].clone())
        z = f(c.noise[rows].clone()) if isinstance(noise, str) else (None if noise is None else f(noise))
        xi = f(c.x_in[rows].clone()) if isinstance(x, str) else (None if x is None else f(x))
        self.flat = {}
        self.flat["counter"], cnt = guarded(dev, (n,), torch.int32, torch.full((n,), c.Ta, dtype=torch.int32) if counter is None else torch.as_tensor(counter, dtype=torch.int32))
        self.flat["chunk"], ch = guarded(dev, (n, c.Ta, c.A), torch.float32, torch.full((n, c.Ta, c.A), POISON) if chunk is None else chunk[rows].clone())
        self.flat["actions"], act = guarded(dev, (n, c.A), torch.float32, POISON)
        self.flat["bad"], bad = guarded(dev, (n,), torch.int32, 99)
        self.flat["x_out"], xo = guarded(dev, (n, c.Ta, c.A), torch.float32, POISON)
        self.flat["noise_out"], no = guarded(dev, (n, c.T + 1, c.Ta, c.A), torch.float32, POISON)
        tw = torch.tensor([t], dtype=torch.int32, device=dev)
        lo, hi, sc, sh = f(pol.lo), f(pol.hi), f(pol.out_scale), f(pol.out_shift)
        a = dict(obs=c.obs, A=c.A, S=c.S, Ta=c.Ta, width=64, heads=4, enc=c.enc, dec=c.dec, T=c.T, linear=1)
        a.update(over)
        ptr = lambda v: None if v is None else v.data_ptr()
        self.rc = capi.load().d3il_ddpm_act_chunk_f32(wn.data_ptr(), lens.data_ptr(), pk["w_in"].data_ptr(), pk["tab"].data_ptr(), pk["enc_w"].data_ptr(), pk["enc_v"].data_ptr(),
                                                      pk["dec_w"].data_ptr(), pk["dec_v"].data_ptr(), pk["head_w"].data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(),
                                                      sh.data_ptr(), seed, env_offset, tw.data_ptr(), ptr(z), ptr(xi), cnt.data_ptr(), ch.data_ptr(), act.data_ptr(), bad.data_ptr(),
                                                      xo.data_ptr(), no.data_ptr(), n, a["obs"], a["A"], a["S"], a["Ta"], a["width"], a["heads"], a["enc"], a["dec"], a["T"], a["linear"],
                                                      k_start, k_stop, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        self.dev_actions = act
        self.actions, self.counter, self.chunk, self.bad, self.x_out, self.noise_out, self.t_word = act.cpu(), cnt.cpu(), ch.cpu(), bad.cpu(), xo.cpu(), no.cpu(), int(tw.item())
        self.sentinels_intact = all(bool((v[:GUARD] == (12345 if v.dtype == torch.int32 else 4242.0)).all() and (v[-GUARD:] == (12345 if v.dtype == torch.int32 else 4242.0)).all())
                                    for v in (w.cpu() for w in self.flat.values()))

    def bits(self):
        return [v.numpy().view(np.uint32) if v.dtype == torch.float32 else v.numpy() for v in (self.actions, self.counter, self.chunk, self.bad, self.x_out, self.noise_out)]


def bar(err_yard, want):
    return 4 * err_yard + 4 * 2.0 ** -24 * float(np.abs(want).max())


@pytest.mark.parametrize("name", list(CASES))
def test_single_chain_steps_within_four_yardsticks_of_f64(dev, name):
    c = case(name)
    for k in sorted({c.T - 1, c.T // 2, 0}, reverse=True):
        want = step_ref(name, k)
        _, t32 = torch_f32(dev, c, x=c.x_in, k_start=k, k_stop=k)
        yard = float(np.abs(t32.double().numpy() - want).max())
        o = Launch(dev, c, x="bank", k_start=k, k_stop=k)
        assert o.rc == 0 and o.sentinels_intact
        err = float(np.abs(o.x_out.double().numpy() - want).max())
        print("%s step %d: kernel %.3e, torch f32 %.3e: %.2f yardsticks, bar %.3e (iterate magnitude %.3e)" % (name, k, err, yard, err / yard, bar(yard, want), float(np.abs(want).max())))
        assert err <= bar(yard, want)
        # the chunk is the final clamp and the two-operation scaling of that iterate, bit for bit; bookkeeping
        pol = c.pol
        y = torch.minimum(torch.maximum(o.x_out, pol.lo), pol.hi) * pol.out_scale + pol.out_shift
        assert np.array_equal(o.chunk.numpy().view(np.uint32), y.numpy().view(np.uint32)) and torch.equal(o.actions, o.chunk[:, 0])
        assert o.counter.tolist() == [1] * N and o.bad.tolist() == [0] * N and o.t_word == 0
        # what was drawn: the bank's row of this step (none at step 0), nothing else
        drawn = torch.full_like(o.noise_out, POISON)
        if k > 0:
            drawn[:, k] = c.noise[:, k]
        assert torch.equal(o.noise_out, drawn)


def test_whole_chain_at_the_small_shape(dev):
    c = case("tiny")
    x = c.noise[:, c.T].double().numpy()
    for i in reversed(range(c.T)):
        x = np.stack([np_step(c, x[r], i, c.win[r, :int(c.len[r])].double().numpy(), c.noise[r, i].double().numpy()) for r in range(N)])
    want = np.clip(x, c.lo64, c.hi64) * c.pol.out_scale.double().numpy() + c.pol.out_shift.double().numpy()
    t32, _ = torch_f32(dev, c)
    yard = float(np.abs(t32.double().numpy() - want).max())
    o = Launch(dev, c)
    assert o.rc == 0 and o.sentinels_intact
    err = float(np.abs(o.chunk.double().numpy() - want).max())
    print("tiny whole chain: kernel %.3e, torch f32 %.3e: %.2f yardsticks, bar %.3e (chunk magnitude %.3e)" % (err, yard, err / yard, bar(yard, want), float(np.abs(want).max())))
    assert err <= bar(yard, want)
    assert float(np.abs(o.x_out.double().numpy() - x).max()) <= bar(float(np.abs(torch_f32(dev, c)[1].double().numpy() - x).max()), x)
    assert torch.equal(o.actions, o.chunk[:, 0]) and o.counter.tolist() == [1] * N and o.bad.tolist() == [0] * N


def test_rows_do_not_depend_on_the_launch(dev):
    c = case("shipped")
    seed, t = 0x1234567890ABCDEF, 7
    whole = Launch(dev, c, noise=None, seed=seed, t=t)
    assert whole.rc == 0 and whole.sentinels_intact and whole.t_word == t      # (the kernel reads the step word; its owner advances it)
    for n in (1, 3, 16):
        part = Launch(dev, c, n=n, noise=None, seed=seed, t=t)
        assert part.sentinels_intact
        for a, b in zip(whole.bits(), part.bits()):
            assert np.array_equal(a[:n], b), n
    off = Launch(dev, c, n=4, rows=slice(5, 9), noise=None, seed=seed, t=t, env_offset=5)
    for a, b in zip(whole.bits(), off.bits()):
        assert np.array_equal(a[5:9], b)
    moved = Launch(dev, c, noise=None, seed=seed, t=t + 1)
    assert not np.isin(moved.noise_out[:, 1:].numpy(), whole.noise_out[:, 1:].numpy()).all()


def _flip(p, Ta):      # another phase: a due lane waits, a waiting lane is due
    return 0 if p == Ta else Ta


@pytest.mark.parametrize("name", ["shipped", "wide"])
def test_a_lane_does_not_depend_on_the_phase_of_its_tile_mates(dev, name):
    c = case(name)
    Ta = c.Ta
    mixed = [(Ta, *range(Ta))[i % (Ta + 1)] for i in range(N)]      # due, 0, 1, .., Ta - 1, due, ..
    X = Launch(dev, c, counter=mixed, chunk=c.prior)
    due = torch.tensor([p == Ta for p in mixed])
    assert X.sentinels_intact and bool(due[:16].any()) and bool((~due[:16]).any())
    # lanes that are not due: chunk, x_out and noise_out untouched, they emit the stored row
    assert np.array_equal(X.chunk[~due].numpy().view(np.uint32), c.prior[~due].numpy().view(np.uint32))
    assert bool((X.x_out[~due] == POISON).all()) and bool((X.noise_out[~due] == POISON).all()) and X.bad.tolist() == [0] * N
    for i in range(N):
        want = X.chunk[i, 0] if mixed[i] == Ta else c.prior[i, mixed[i]]
        assert torch.equal(X.actions[i], want) and int(X.counter[i]) == (1 if mixed[i] == Ta else mixed[i] + 1)
    for keep in (0, 1):      # the lanes of one parity keep their phase, their tile-mates take another one
        other = [p if i % 2 == keep else _flip(p, Ta) for i, p in enumerate(mixed)]
        Y = Launch(dev, c, counter=other, chunk=c.prior)
        sel = (torch.arange(N) % 2 == keep).numpy()
        for a, b in zip(X.bits(), Y.bits()):
            assert np.array_equal(a[sel], b[sel])
    # and equal to the launch in which every lane is due
    full = Launch(dev, c, chunk=c.prior)
    assert np.array_equal(X.chunk[due].numpy().view(np.uint32), full.chunk[due].numpy().view(np.uint32)) and full.counter.tolist() == [1] * N
    # no lane due: the network is skipped, only actions, counters and the zero marks are written, the windows are not read
    waiting = [i % Ta for i in range(N)]
    Z = Launch(dev, c, counter=waiting, chunk=c.prior, win=torch.full_like(c.win, float("nan")))
    assert Z.sentinels_intact and np.array_equal(Z.chunk.numpy().view(np.uint32), c.prior.numpy().view(np.uint32))
    assert bool((Z.x_out == POISON).all()) and bool((Z.noise_out == POISON).all()) and Z.bad.tolist() == [0] * N
    assert torch.equal(Z.actions, c.prior[torch.arange(N), torch.tensor(waiting)]) and Z.counter.tolist() == [w + 1 for w in waiting]


def test_a_lane_does_not_depend_on_the_window_length_of_its_tile_mates(dev):
    c = case("shipped")
    base = Launch(dev, c)
    other = c.len.clone()
    win = c.win.clone()
    odd = torch.arange(N) % 2 == 1
    other[odd] = 1      # the odd lanes shrink to one window row (their later rows become padding)
    win[odd, 1:] = 0.0
    moved = Launch(dev, c, ln=other, win=win)
    even = (~odd).numpy()
    for a, b in zip(base.bits(), moved.bits()):
        assert np.array_equal(a[even], b[even])
    assert not np.array_equal(base.chunk[odd & (c.len > 1)].numpy(), moved.chunk[odd & (c.len > 1)].numpy())


def test_noise_is_the_host_philox_and_the_first_iterate_is_the_noise(dev):
    from d3il_amd import policies as P
    c = case("wide")      # A = 8: both calls q of every (token, chain index)
    seed, t = 0xFEDCBA9876543210, 3
    o = Launch(dev, c, noise=None, seed=seed, t=t)
    host = np.stack([np.zeros((N, c.Ta, c.A))] + [P.ddpm_act_normals(seed, 0, N, t, k, c.Ta, c.A) for k in range(1, c.T + 1)], axis=1)
    # the yardstick: torch's f32 Box-Muller on the same words, on the device
    w = torch.as_tensor(np.stack([P.ddpm_act_words(seed, 0, N, t, k, c.Ta) for k in range(1, c.T + 1)], axis=1).astype(np.int64)).to(dev)
    u1 = ((w[..., 0::2] >> 8).float() + 1.0) * (1.0 / 16777216.0)
    u2 = (w[..., 1::2] >> 8).float() * (1.0 / 16777216.0)
    rad = torch.sqrt(-2.0 * torch.log(u1))
    t32 = torch.stack((rad * torch.cos(6.283185307179586 * u2), rad * torch.sin(6.283185307179586 * u2)), dim=-1).reshape(N, c.T, c.Ta, 8).cpu().double().numpy()
    yard = float(np.abs(t32 - host[:, 1:]).max())
    err = float(np.abs(o.noise_out[:, 1:].double().numpy() - host[:, 1:]).max())
    print("noise_out against the host form: %.3e, torch f32 Box-Muller %.3e: %.2f yardsticks" % (err, yard, err / yard))
    assert err <= 4 * yard and bool((o.noise_out[:, 0] == POISON).all())      # chain index 0 is never drawn
    # no step at all: the first iterate is the drawn noise, bit for bit, and goes to the final clamp
    first = Launch(dev, c, noise=None, seed=seed, t=t, k_start=c.T - 1, k_stop=c.T)
    assert np.array_equal(first.x_out.numpy().view(np.uint32), o.noise_out[:, c.T].numpy().view(np.uint32)) and np.array_equal(first.noise_out[:, c.T].numpy(), o.noise_out[:, c.T].numpy())
    assert bool((first.noise_out[:, :c.T] == POISON).all())
    # the offset reaches the high counter word
    far = Launch(dev, c, n=2, noise=None, seed=seed, t=t, env_offset=(1 << 32) - 1, k_start=c.T - 1, k_stop=c.T)
    want = P.ddpm_act_normals(seed, (1 << 32) - 1, 2, t, c.T, c.Ta, c.A)
    assert float(np.abs(far.x_out.double().numpy() - want).max()) <= 4 * yard


def test_step_zero_reads_no_noise(dev):
    c = case("shipped")
    base = Launch(dev, c, x="bank", k_start=0, k_stop=0)
    loud = c.noise.clone()
    loud[:, 0] = 1e30
    other = Launch(dev, c, x="bank", k_start=0, k_stop=0, noise=loud)
    for a, b in zip(base.bits(), other.bits()):
        assert np.array_equal(a, b)
    whole, whole_loud = Launch(dev, c), Launch(dev, c, noise=loud)
    for a, b in zip(whole.bits(), whole_loud.bits()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["shipped", "wide"])
def test_nonfinite_values_mark_their_lane_only(dev, name):
    c = case(name)
    clean = Launch(dev, c, chunk=c.prior)
    assert clean.bad.tolist() == [0] * N
    # padding rows filled with NaN change nothing and mark nothing
    pad = c.win.clone()
    for i in range(N):
        pad[i, int(c.len[i]):] = float("nan")
    padded = Launch(dev, c, chunk=c.prior, win=pad)
    assert bool((c.len < c.S).any())
    for a, b in zip(clean.bits(), padded.bits()):
        assert np.array_equal(a, b)
    # a NaN and an Inf in a valid window row of a due lane
    win = c.win.clone()
    win[3, 0, 1], win[16, int(c.len[16]) - 1, c.obs - 1] = float("nan"), float("inf")      # (lane 16: the tail tile)
    bad = Launch(dev, c, win=win, chunk=c.prior)
    hit = [3, 16]
    good = [r for r in range(N) if r not in hit]
    assert bad.sentinels_intact and torch.isnan(bad.chunk[hit]).all() and torch.isnan(bad.actions[hit]).all() and bad.counter.tolist() == [1] * N
    assert bad.bad.tolist() == [int(r in hit) for r in range(N)]
    assert bool((bad.chunk[hit].view(torch.int32) == 0x7FC00000).all()) and bool((bad.actions[hit].view(torch.int32) == 0x7FC00000).all())
    for a, b in zip(bad.bits()[:4], clean.bits()[:4]):
        assert np.array_equal(a[good], b[good])
    # ... and of a waiting lane: nothing changes
    cnt = [c.Ta if i % 2 == 0 else 0 for i in range(N)]
    base = Launch(dev, c, counter=cnt, chunk=c.prior)
    win = c.win.clone()
    win[5, 0, 0], win[7, 0, 2] = float("nan"), float("inf")
    same = Launch(dev, c, counter=cnt, chunk=c.prior, win=win)
    for a, b in zip(base.bits(), same.bits()):
        assert np.array_equal(a, b)
    # an Inf reached mid-chain (the noise of a middle step) marks only its lane
    mid = max(1, c.T // 2)
    noise = c.noise.clone()
    noise[6, mid, c.Ta - 1, c.A - 1] = float("inf")
    late = Launch(dev, c, noise=noise, chunk=c.prior)
    good = [r for r in range(N) if r != 6]
    assert late.bad.tolist() == [int(r == 6) for r in range(N)] and torch.isnan(late.chunk[6]).all() and torch.isnan(late.actions[6]).all()
    for a, b in zip(late.bits()[:5], clean.bits()[:5]):
        assert np.array_equal(a[good], b[good])


def test_unsupported_shapes_are_refused_before_any_launch(dev):
    c = case("shipped")
    for kw in (dict(width=128), dict(heads=8), dict(obs=33), dict(obs=0), dict(A=9), dict(A=0), dict(S=6), dict(S=0), dict(Ta=5), dict(Ta=0), dict(enc=5), dict(enc=0), dict(dec=9),
               dict(dec=0), dict(T=256), dict(T=0), dict(linear=0)):
        o = Launch(dev, c, n=4, **kw)
        assert o.rc == EUNSUPPORTED, kw
        assert o.sentinels_intact and o.counter.tolist() == [c.Ta] * 4 and o.bad.tolist() == [99] * 4, kw
        assert all(bool((v == POISON).all()) for v in (o.actions, o.chunk, o.x_out, o.noise_out)), kw
    ok = Launch(dev, c, n=4)
    assert ok.rc == 0 and ok.counter.tolist() == [1] * 4 and torch.isfinite(ok.chunk).all()


def test_other_shapes_take_the_torch_path(dev, monkeypatch):
    """A width the kernel is not built for: the policy does not call the entry (which would refuse) but runs the torch path, on the device, on the same Philox stream."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
    pol = P.DDPMACTPolicy.random(4, 2, device=dev, seed=2, enc_layers=1, dec_layers=1, embed_dim=128, n_timesteps=3, policy_seed=3)
    pol.record = True
    obs = torch.randn(3, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    assert not pol.fused_ok(obs)
    with pytest.warns(UserWarning, match="torch path"):
        y = pol.predict_batch(obs)
    assert y.shape == (3, 2) and torch.isfinite(y).all() and pol._packed.key is None and pol.counter.tolist() == [1, 1, 1]
    assert np.array_equal(pol.last_noise[:, 3].cpu().numpy(), P.ddpm_act_normals(3, 0, 3, 0, 3, 4, 2).astype(np.float32))


def test_the_step_word_advances_once_per_call(dev, monkeypatch):
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
    pol = P.DDPMACTPolicy.random(4, 2, device=dev, seed=11, obs_seq_len=1, action_seq_len=1, enc_layers=1, dec_layers=1, n_timesteps=2, policy_seed=5)      # Ta = 1: every call draws
    pol.record = True
    obs = case("tiny").win[:, 0].to(dev)
    for t in range(3):
        assert pol.fused_ok(obs)
        pol.predict_batch(obs)
        want = P.ddpm_act_normals(5, 0, N, t, 2, 1, 2)
        assert int(pol._t) == t + 1 and float(np.abs(pol.last_noise[:, 2].cpu().double().numpy() - want).max()) <= 1e-5 and not bool(pol.last_bad.any())
