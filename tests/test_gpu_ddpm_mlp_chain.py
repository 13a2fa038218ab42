"""d3il_ddpm_mlp_chain (csrc/policy_ddpm_mlp.h) on the GPU against an f64 NumPy restatement of the chain on the same f32 inputs (state rows, weights, the time
embeddings, the schedule table, bounds, scaling, the noise bank).  The yardstick of every accuracy assertion is the deviation torch's own f32
chain - F.linear on the unsplit input row [x | temb[i] | s], F.mish, the update - shows against the f64 result on the same rows, computed per case and printed;
the kernel has to stay within 4 of it.  One workgroup serves 16 rows and the grid is not capped: launches of 1, 15, 16 and 17 rows must equal the first rows of the
257-row launch bit for bit.

The bounds of the cases are +-10 in scaled space, not the +-1.5 of the ``random()`` policies, so that the yardstick is one.  At the first reverse step x0 = sra x - srm1
eps with sra, srm1 of 20 .. 30 (T = 4; 31.6 at T = 1): against bounds of +-1.5 all but a few rows are clipped there, the rows that escape carry the f32 error of their
eps times srm1, and the largest error of a case is the maximum over a handful of values - between two f32 evaluations of the SAME chain by torch (F.linear on the unsplit
input row against the policy's own split order) it differs by factors of 0.19 .. 3.56 over these 41 cases, on the host, no kernel involved.  Against +-10 a sixth to a
half of the rows escape, the maximum is taken over a population, and the same two torch evaluations agree within 0.65 .. 1.43 in every case; the clip still acts on
the rest, and the final clamp on a share that every case asserts."""
import copy
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 257
SHAPES = ((2, 4, 10), (3, 8, 20), (8, 4, 20), (2, 24, 4), (8, 16, 40))      # (A, t_dim, obs): 16, 31, 32, 30 and exactly 64 input columns; one and two Philox calls
# name: (hidden, A, t_dim, obs, residual blocks, T)
CASES = {"h%d_a%d_t%d_o%d_b%d_T%d" % (h, A, td, obs, b, T): (h, A, td, obs, b, T) for h, (A, td, obs), b, T in itertools.product((128, 256), SHAPES, (0, 3), (1, 4))}
CASES["h128_a3_t8_o20_b3_T24"] = (128, 3, 8, 20, 3, 24)
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def mish64(x):
    return x * np.tanh(np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0)))))


def chain64(pol, temb, sched, state, noise):
    """The chain of ``pol`` in f64 NumPy on the f32 inputs (host tensors), the input layer unsplit: (actions [n, A], the final x in front of its clamp)."""
    d = lambda t: t.detach().double().cpu().numpy()
    lin_in, blocks, lin_out = pol.model.layers._parts()
    W, b, temb, sch = d(lin_in.weight), d(lin_in.bias), d(temb), d(sched)
    lo, hi, sc, sh = d(pol.lo), d(pol.hi), d(pol.out_scale), d(pol.out_shift)
    s, z = d(state), d(noise)
    x = z[0]
    for step in range(pol.T):
        i = pol.T - 1 - step
        h = np.concatenate([x, np.broadcast_to(temb[i], (len(s), pol.t_dim)), s], axis=1) @ W.T + b
        for l1, l2 in blocks:
            h = h + mish64(mish64(h) @ d(l1.weight).T + d(l1.bias)) @ d(l2.weight).T + d(l2.bias)
        eps = h @ d(lin_out.weight).T + d(lin_out.bias)
        x0 = np.clip(sch[i, 0] * x - sch[i, 1] * eps, lo, hi)
        x = sch[i, 2] * x0 + sch[i, 3] * x
        if i > 0:
            x = x + sch[i, 4] * z[step + 1]
    return np.clip(x, lo, hi) * sc + sh, x


def chain32(pol, temb, sched, state, noise):
    """torch's own f32 chain on the same rows (all on one device): F.linear on the unsplit input row, F.mish, the update, the tail."""
    F = torch.nn.functional
    lin_in, blocks, lin_out = pol.model.layers._parts()
    with torch.no_grad():
        x = noise[0]
        for step in range(pol.T):
            i = pol.T - 1 - step
            h = F.linear(torch.cat([x, temb[i].expand(len(state), -1), state], dim=1), lin_in.weight, lin_in.bias)
            for l1, l2 in blocks:
                h = h + F.linear(F.mish(F.linear(F.mish(h), l1.weight, l1.bias)), l2.weight, l2.bias)
            eps = F.linear(h, lin_out.weight, lin_out.bias)
            x0 = torch.minimum(torch.maximum(sched[i, 0] * x - sched[i, 1] * eps, pol.lo), pol.hi)
            x = sched[i, 2] * x0 + sched[i, 3] * x
            if i > 0:
                x = x + sched[i, 4] * noise[step + 1]
        return torch.minimum(torch.maximum(x, pol.lo), pol.hi) * pol.out_scale + pol.out_shift


class Case:
    """A random-weight policy on the host (its packed tables are the kernel's inputs), scaled state rows, a noise bank [T + 1, N, A] (entry T is the step the chain never
    draws), and - computed once - the f64 result and torch's f32 result on the same rows."""

    def __init__(self, name):
        from d3il_amd import policies as P
        self.name = name
        self.hidden, self.A, self.td, self.obs, self.nblk, self.T = CASES[name]
        i = list(CASES).index(name)
        self.pol = P.DDPMNativePolicy.random(self.obs, self.A, device="cpu", seed=60 + i, hidden_dim=self.hidden, n_blocks=self.nblk, t_dim=self.td, n_timesteps=self.T,
                                             action_scale=0.004, bound=10.0)
        self.pol.out_shift = (torch.arange(self.A, dtype=torch.float32) * 0.001 - 0.003).contiguous()      # a shift, so that the inverse scaling is a product AND a sum
        with torch.no_grad():      # a noise estimate of a few tenths to about one: the x0 clip and the final clamp both act, neither on every row
            self.pol.model.layers.layers[-1].weight.mul_(4.0)
        g = torch.Generator().manual_seed(160 + i)
        self.state = torch.randn(N, self.obs, generator=g) * 0.8
        self.noise = torch.randn(self.T + 1, N, self.A, generator=g)
        self.pk = self.pol._pack()
        self.want, self.x_final = self.chain64(self.state, self.noise)
        self.t32 = self.chain32(self.state, self.noise)
        self.yard = float(np.abs(self.t32.double().numpy() - self.want).max())
        self.dpk = None

    def chain64(self, state, noise, sched=None):
        return chain64(self.pol, self.pk["temb"], self.pk["sched"] if sched is None else sched, state, noise)

    def chain32(self, state, noise):
        return chain32(self.pol, self.pk["temb"], self.pk["sched"], state, noise)

    def packed(self, dev):
        if self.dpk is None:
            self.dpk = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in self.pk.items()}
        return self.dpk


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


class Launch:
    """One call of the entry point.  ``noise``: "bank" = the case's bank, None = Philox, or a tensor [>= T, N, A].  Outputs are filled with 777 before the call."""

    def __init__(self, dev, c, n=N, first=0, state=None, noise="bank", seed=0, t=0, env_offset=0, noise_out=True, sched=None, **over):
        from d3il_amd import capi
        pk = c.packed(dev)
        hidden, A, td, obs, nblk, T = (over.get(k, d) for k, d in (("hidden", c.hidden), ("A", c.A), ("td", c.td), ("obs", c.obs), ("nblk", c.nblk), ("T", c.T)))
        st = (c.state if state is None else state)[first:first + n].to(dev).contiguous()
        nz = c.noise if isinstance(noise, str) else noise
        nz = None if nz is None else nz[:, first:first + n].to(dev).contiguous()
        word = torch.tensor([t], dtype=torch.int64, device=dev).to(torch.int32)
        f = lambda v: v.to(dev).contiguous()
        sch = pk["sched"] if sched is None else f(sched)
        self.keep = (f(c.pol.lo), f(c.pol.hi), f(c.pol.out_scale), f(c.pol.out_shift), st, nz, word, sch)
        lo, hi, sc, sh = self.keep[:4]
        act = torch.full((n, 8), 777.0, device=dev)[:, :max(c.A, 1)].contiguous()
        bad = torch.full((n,), 777, dtype=torch.int32, device=dev)
        no = torch.full((c.T + 1, n, c.A), 777.0, device=dev)
        self.rc = capi.load().d3il_ddpm_mlp_chain(word.data_ptr(), st.data_ptr(), pk["w_x"].data_ptr(), pk["w_state"].data_ptr(), pk["tbias"].data_ptr(), pk["w_blk"].data_ptr(),
                                                  pk["b_blk"].data_ptr(), pk["w_out"].data_ptr(), pk["b_out"].data_ptr(), sch.data_ptr(), lo.data_ptr(), hi.data_ptr(), sc.data_ptr(),
                                                  sh.data_ptr(), seed, env_offset, None if nz is None else nz.data_ptr(), act.data_ptr(), bad.data_ptr(),
                                                  no.data_ptr() if noise_out else None, n, obs, A, td, T, hidden, nblk, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        self.actions, self.bad, self.noise_out = act.cpu(), bad.cpu(), no.cpu()

    def bits(self):
        return self.actions.numpy().view(np.uint32), self.noise_out.numpy().view(np.uint32), self.bad.numpy()


def same(a, b, rows=slice(None)):
    """Bit for bit: actions, noise_out, bad of launch a against the rows of launch b."""
    (aa, an, ab), (ba, bn, bb) = a.bits(), b.bits()
    return np.array_equal(aa, ba[rows]) and np.array_equal(an, bn[:, rows]) and np.array_equal(ab, bb[rows])


@pytest.mark.parametrize("name", list(CASES))
def test_actions_against_f64_and_rows_do_not_depend_on_the_launch(dev, name):
    c = case(name)
    out = Launch(dev, c)
    assert out.rc == 0 and not out.bad.any()
    lo, hi = c.pol.lo.double().numpy(), c.pol.hi.double().numpy()
    inside = float(np.mean((c.x_final > lo) & (c.x_final < hi)))
    err = float(np.abs(out.actions.double().numpy() - c.want).max())
    print("%s: kernel %.3e, torch f32 %.3e -> %.2f yardsticks (%.2f of the final x strictly inside the bounds; largest action %.3e)"
          % (name, err, c.yard, err / c.yard, inside, float(np.abs(c.want).max())))
    assert c.yard > 0 and err <= 4 * c.yard
    if c.T <= 4:      # a sizeable share inside, and the clamp acts (T = 24: the long chain ends inside throughout)
        assert 0.1 < inside < 1.0
    # noise_out: what was used, zeros for the step that draws nothing; without noise_out: the same actions
    assert torch.equal(out.noise_out[:c.T], c.noise[:c.T]) and not out.noise_out[c.T].any()
    assert np.array_equal(Launch(dev, c, noise_out=False).bits()[0], out.bits()[0])
    # 1, 15, 16 and 17 rows: the first rows of the 257-row launch, bit for bit
    for n in (1, 15, 16, 17):
        assert same(Launch(dev, c, n=n), out, slice(0, n)), n


@pytest.mark.parametrize("name", ["h128_a2_t24_o4_b3_T4", "h256_a8_t16_o40_b0_T4"])
def test_the_bank_entry_of_the_last_step_is_never_read(dev, name):
    c = case(name)
    out = Launch(dev, c)
    noise = c.noise.clone()
    noise[c.T] = float("nan")
    noise[c.T, ::2] = 1e30
    assert same(Launch(dev, c, noise=noise), out)
    assert same(Launch(dev, c, noise=c.noise[:c.T].clone()), out)      # a bank of T entries is all the entry needs


def test_clamp_edges_are_exact(dev):
    """T = 1 with the schedule row (sra, srm1, c1, c2, sig) = (2, 1, c1, 0, 0) and eps of +-100: x0 is clipped to hi / lo; with c1 = 1 the final x sits exactly on the
    bound and the final clamp keeps it, with c1 = 3 it lies beyond and the final clamp puts it on the bound - both come out as (bound scale) + shift, product and
    sum in f32, bit for bit."""
    c = copy.copy(case("h128_a8_t4_o20_b3_T1"))
    c.pol = copy.copy(c.pol)
    c.pol.model = copy.deepcopy(c.pol.model)
    c.pol._packed = type(c.pol._packed)()
    with torch.no_grad():
        c.pol.model.layers.layers[-1].weight.zero_()
        c.pol.model.layers.layers[-1].bias.copy_(torch.tensor([100.0, -100.0] * 4))      # x0 = 2 x - eps: below lo in the even components, above hi in the odd ones
    c.pk, c.dpk = c.pol._pack(), None
    p = c.pol
    want = torch.where(torch.arange(8) % 2 == 0, p.lo * p.out_scale + p.out_shift, p.hi * p.out_scale + p.out_shift).expand(N, 8).contiguous()
    for c1 in (1.0, 3.0):
        out = Launch(dev, c, sched=torch.tensor([[2.0, 1.0, c1, 0.0, 0.0]]))
        assert out.rc == 0 and not out.bad.any()
        assert np.array_equal(out.actions.numpy().view(np.uint32), want.numpy().view(np.uint32)), c1
    # and a final x strictly inside stays what it is: c1 = 0.5 puts it at half the bound
    out = Launch(dev, c, sched=torch.tensor([[2.0, 1.0, 0.5, 0.0, 0.0]]))
    half = torch.where(torch.arange(8) % 2 == 0, (0.5 * p.lo) * p.out_scale + p.out_shift, (0.5 * p.hi) * p.out_scale + p.out_shift).expand(N, 8).contiguous()
    assert np.array_equal(out.actions.numpy().view(np.uint32), half.numpy().view(np.uint32))


@pytest.mark.parametrize("name", ["h128_a2_t4_o10_b3_T4", "h256_a8_t4_o20_b3_T4", "h128_a3_t8_o20_b0_T1"])
def test_philox_stream(dev, name):
    """noise_in NULL: noise_out is ddpm_mlp_normals on the host to f32 Box-Muller accuracy (yardstick: torch's f32 Box-Muller on the same words against f64), at a
    non-zero env_offset, a non-zero step word and a seed beyond 32 bits; the actions are the chain's on that noise; rows 5 .. 8 equal a 4-row launch at env_offset + 5."""
    from d3il_amd import policies as P
    c = case(name)
    seed, t, off = 0x1234567890ABCDEF, 0x80000007, (1 << 32) + 1000
    out = Launch(dev, c, n=40, noise=None, seed=seed, t=t, env_offset=off)
    assert out.rc == 0 and not out.bad.any() and not out.noise_out[c.T].any()
    for k in range(c.T):
        want = P.ddpm_mlp_normals(seed, off, 40, t, k, c.A)
        r = torch.as_tensor(P.ddpm_mlp_words(seed, off, 40, t, k).astype(np.int64))
        u1, u2 = ((r[..., 0::2] >> 8) + 1).float() * 2.0 ** -24, (r[..., 1::2] >> 8).float() * 2.0 ** -24      # [n, q, pair]
        rad, ang = torch.sqrt(-2.0 * torch.log(u1)), 6.28318530717958647692 * u2
        t32 = torch.stack((rad * torch.cos(ang), rad * torch.sin(ang)), dim=-1).reshape(40, 8)[:, :c.A]
        yard = float(np.abs(t32.double().numpy() - want).max())
        err = float(np.abs(out.noise_out[k].double().numpy() - want).max())
        print("%s draw %d: kernel %.3e torch f32 %.3e -> %.2f yardsticks" % (name, k, err, yard, err / yard))
        assert yard > 0 and err <= 4 * yard
    # the actions are the chain's on that noise: the same launch with noise_out handed back as noise_in
    again = Launch(dev, c, n=40, noise=out.noise_out.clone())
    assert np.array_equal(again.bits()[0], out.bits()[0])
    part = Launch(dev, c, n=4, first=5, noise=None, seed=seed, t=t, env_offset=off + 5)
    assert same(part, out, slice(5, 9))
    # another step word, another seed, another offset: other draws
    for kw in (dict(seed=seed, t=t + 1, env_offset=off), dict(seed=seed + 1, t=t, env_offset=off), dict(seed=seed, t=t, env_offset=off + 1)):
        assert not np.array_equal(Launch(dev, c, n=40, noise=None, **kw).bits()[1][:c.T], out.bits()[1][:c.T])
    # no word of the other policies' streams for the same (seed, env, t)
    mine = np.concatenate([P.ddpm_mlp_words(seed, off, 40, t, k).reshape(40, -1) for k in range(c.T)], axis=1)
    others = np.concatenate([P.ddpm_gpt_words(seed, off, 40, t, k, 16).reshape(40, -1) for k in (1, 2, 255)] + [P.cvae_words(seed, off, 40, t).reshape(40, -1),
                             P.bet_mlp_words(seed, off, 40, t).reshape(40, -1), P.beso_words(seed, off, 40, t, 1, 16).reshape(40, -1)], axis=1)
    assert not np.intersect1d(mine.ravel(), others.ravel()).size


@pytest.mark.parametrize("name", ["h128_a3_t8_o20_b3_T4", "h256_a8_t16_o40_b3_T4"])
def test_a_non_finite_row_is_marked_and_its_neighbours_do_not_change(dev, name):
    c = copy.copy(case(name))
    c.pol = copy.copy(c.pol)
    c.pol.model = copy.deepcopy(c.pol.model)
    with torch.no_grad():      # every hidden unit reads the first state feature with weight 4: a row whose feature is 3e38 overflows in the input layer, no other row does
        c.pol.model.layers.layers[0].weight[:, c.A + c.td] = 4.0
    c.pk, c.dpk = c.pol._pack(), None
    clean = Launch(dev, c, n=40)
    assert clean.rc == 0 and not clean.bad.any()
    ca, cn, cb = clean.bits()
    others = np.array([r for r in range(40) if r != 17])
    plants = []
    for v in (float("nan"), float("inf"), -float("inf")):
        st = c.state.clone(); st[17, c.obs - 1] = v
        plants.append(("state %r" % v, dict(state=st)))
    for k in range(c.T):      # every draw the chain uses, first and last component
        nz = c.noise.clone(); nz[k, 17, (0, c.A - 1)[k % 2]] = float("nan") if k % 2 else float("inf")
        plants.append(("draw %d" % k, dict(noise=nz)))
    st = c.state.clone(); st[17, 0] = 3.0e38      # finite, and 4 x 3e38 overflows in the input layer: the row's hidden units, its eps and its final x are not finite
    plants.append(("overflow", dict(state=st)))
    for what, kw in plants:
        out = Launch(dev, c, n=40, **kw)
        a, _, b = out.bits()
        assert out.rc == 0 and b.tolist() == [int(r == 17) for r in range(40)], what
        assert (a[17] == 0x7FC00000).all(), what
        assert np.array_equal(a[others], ca[others]), what


def test_refusals_leave_the_outputs_alone(dev):
    c = case("h128_a2_t4_o10_b3_T4")
    for kw, rc in ((dict(hidden=192), -5), (dict(A=9), -5), (dict(A=0), -5), (dict(obs=59), -5), (dict(td=53), -5), (dict(obs=0), -5), (dict(T=256), -5), (dict(T=0), -1),
                   (dict(nblk=-1), -5)):      # (obs 59: 2 + 4 + 59 = 65 input columns)
        o = Launch(dev, c, n=4, **kw)
        assert o.rc == rc, kw
        assert (o.actions == 777.0).all() and (o.bad == 777).all() and (o.noise_out == 777.0).all(), kw
    from d3il_amd import capi
    assert b"d3il_ddpm_mlp_chain" in capi.load().d3il_last_error()
