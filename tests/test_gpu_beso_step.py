"""k_beso_step (csrc/policy_beso.h) through d3il_beso_step on the GPU against an f64 NumPy restatement of its steps (LayerNorm, the linear head, the Karras
combination, the derivative, the Euler step, the ancestral noise, the next iterate, its action tokens + the sigma token; at the last step the clamped scaled action, the
inverse-scaled action and the ring push; in init mode the first iterate from the action ring and one draw).

Geometry (a launch gets one workgroup of four waves per 4 environments, at most 1024 workgroups; one wave owns one environment at a time and walks its W positions,
every wave takes its environments in a block-stride loop): n_env 1 (three idle waves), 63 (the last workgroup with three live waves), 64, 65 (a workgroup with one
live wave), 257 and 8200 (the capped grid: 4096 waves, three passes, the third with 8 live waves).  C in {72, 120} are the compile-time widths, C in {32, 100, 128} run the run-time instantiation;
A in {2, 3, 8}; W in {1, 5}; step index i in {-1 (init), 0, a middle step, S - 1}; ragged lengths 1 .. W.

The bar (DESIGN sections 26.3 / 28): every value within 4 x the deviation of torch's own f32 layer_norm + F.linear + update chain from f64 on the same rows, computed per
case and never carried over."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S = 16
MID = 7
SOLVER_FAIL = 1 << 16
SENT = 777.0
SIGMA_MIN, SIGMA_MAX, SIGMA_DATA = 0.01, 0.8, 0.5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def tables(s):
    """(coef [s, 6] f32, c_in0) of the linear schedule SIGMA_MAX .. SIGMA_MIN in s steps: the policy's own host code."""
    from d3il_amd import policies as P
    sig = torch.cat([torch.linspace(SIGMA_MAX, SIGMA_MIN, s), torch.zeros(1)]).tolist()
    rows, c_in0 = P.beso_coefficients(sig, SIGMA_DATA)
    return np.asarray(rows, dtype=np.float64).astype(np.float32), float(np.float32(c_in0))


def make_case(n, W, Cw, A, seed, s=S):
    """Host arrays (f32) of one problem: hidden rows, ln_f, head, action embedding, tables, bounds, scaling, ragged lengths, iterate, action ring, noise."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    coef, c_in0 = tables(s)
    return dict(hk=f(rng.normal(size=(n, W, Cw)) * 1.7 + 0.3), ln_w=f(1.0 + 0.3 * rng.normal(size=Cw)), ln_b=f(0.2 * rng.normal(size=Cw)), eps=1e-5,
                w_pred=f(rng.normal(size=(A, Cw)) / np.sqrt(Cw)), b_pred=f(0.1 * rng.normal(size=A)), w_aemb=f(rng.normal(size=(Cw, A)) * 0.3),
                bias_pos=f(rng.normal(size=(W, Cw)) * 0.2), semb=f(rng.normal(size=(s, Cw)) * 0.5), coef=coef, c_in0=c_in0, sigma_max=float(np.float32(SIGMA_MAX)), S=s,
                lo=f(-1.2 - 0.3 * rng.random(A)), hi=f(1.2 + 0.3 * rng.random(A)), scale=f(0.004 * (1 + rng.random(A))), shift=f(0.001 * rng.normal(size=A)),
                len=np.ascontiguousarray(1 + (np.arange(n) * 7 + seed) % W, dtype=np.int64), x=f(rng.normal(size=(n, W, A))), ring=f(rng.normal(size=(n, W - 1, A))),
                noise=f(rng.normal(size=(n, W, A))))


def first_rows(c, n):
    """The case cut down to its first n environments."""
    return dict(c, **{q: np.ascontiguousarray(c[q][:n]) for q in ("hk", "len", "x", "ring", "noise")})


def first_iterate(c, xp_newest):
    """Init mode's x': ring entries (W - 1) - (len - 1) + j at j < len - 1, ``xp_newest`` [n, A] at len - 1, 0 behind (dtype of xp_newest)."""
    n, W, A = c["x"].shape
    xp = np.zeros((n, W, A), dtype=xp_newest.dtype)
    for e in range(n):
        L = int(c["len"][e])
        for j in range(L - 1):
            xp[e, j] = c["ring"][e, (W - 1) - (L - 1) + j]
        xp[e, L - 1] = xp_newest[e]
    return xp


def step64(c, i, noise=None, hk=None, x=None):
    """The steps in f64 on the f32 inputs: dict(xp [n, W, A], tok [n, W, C], valid [n, W]; at i = S - 1 also a_new [n, A], actions [n, A], ring [n, W - 1, A])."""
    d = lambda a: np.asarray(a, dtype=np.float64)
    n, W, A = c["x"].shape
    noise = d(c["noise"] if noise is None else noise)
    valid = np.arange(W)[None, :] < c["len"][:, None]
    last = i == c["S"] - 1
    if i < 0:
        xp = first_iterate(c, d(c["sigma_max"]) * noise[:, 0])
        c_in = d(c["c_in0"])
    else:
        h, x = d(c["hk"] if hk is None else hk), d(c["x"] if x is None else x)
        mu = h.mean(2, keepdims=True)
        z = (h - mu) / np.sqrt(((h - mu) ** 2).mean(2, keepdims=True) + c["eps"]) * d(c["ln_w"]) + d(c["ln_b"])
        net = z @ d(c["w_pred"]).T + d(c["b_pred"])
        k = d(c["coef"][i])
        den = k[1] * net + k[0] * x
        xp = x + (x - den) * k[2] * k[3]
        if not last:
            xp = xp + k[4] * noise
        c_in = k[5]
    xp = np.where(valid[:, :, None], xp, 0.0)
    out = dict(xp=xp, valid=valid, tok=(c_in * xp) @ d(c["w_aemb"]).T + d(c["bias_pos"]))
    if last:
        out["a_new"] = np.clip(xp[np.arange(n), c["len"] - 1], d(c["lo"]), d(c["hi"]))
        out["actions"] = out["a_new"] * d(c["scale"]) + d(c["shift"])
        out["ring"] = np.concatenate((d(c["ring"])[:, 1:], out["a_new"][:, None]), axis=1) if W > 1 else d(c["ring"])
    return out


def torch_f32(dev, c, i):
    """torch's own f32 layer_norm + F.linear + update chain on the same device for the same case: (xp, tok, a_new or None, actions or None) as f64 host arrays."""
    F = torch.nn.functional
    d = lambda a: torch.as_tensor(a).to(dev)
    n, W, A = c["x"].shape
    valid = (torch.arange(W, device=dev)[None, :] < d(c["len"])[:, None]).unsqueeze(2)
    last = i == c["S"] - 1
    if i < 0:
        xp = d(first_iterate(c, (torch.tensor(c["sigma_max"]) * torch.as_tensor(c["noise"][:, 0])).numpy()))
        c_in = torch.tensor(c["c_in0"], device=dev)
    else:
        z = F.layer_norm(d(c["hk"]), (c["hk"].shape[2],), d(c["ln_w"]), d(c["ln_b"]), c["eps"])
        net = F.linear(z, d(c["w_pred"]), d(c["b_pred"]))
        k, x = d(c["coef"][i]), d(c["x"])
        den = k[1] * net + k[0] * x
        xp = x + (x - den) * k[2] * k[3]
        if not last:
            xp = xp + k[4] * d(c["noise"])
        c_in = k[5]
    xp = torch.where(valid, xp, torch.zeros_like(xp))
    tok = F.linear(c_in * xp, d(c["w_aemb"])) + d(c["bias_pos"])
    a_new = act = None
    if last:
        newest = xp[torch.arange(n, device=dev), d(c["len"]) - 1]
        a32 = torch.minimum(torch.maximum(newest, d(c["lo"])), d(c["hi"]))
        a_new, act = a32.double().cpu().numpy(), (a32 * d(c["scale"]) + d(c["shift"])).double().cpu().numpy()
    return xp.double().cpu().numpy(), tok.double().cpu().numpy(), a_new, act


class Launch:
    """One call of d3il_beso_step on device copies of a case; results as host arrays.  Every pointer handed over is kept alive until the results are read.
    ``state``: (x, xbuf, ring, actions, bad) device tensors of an earlier launch to go on with (a chain), otherwise fresh ones (sentinels where the launch writes)."""

    def __init__(self, dev, c, i, noise="case", seed=0, env_offset=0, t=0, t_dev=None, hk=None, x=None, state=None, want_noise=True, C_=None, A_=None, W_=None, S_=None, n_=None):
        from d3il_amd import capi
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
        n, W, A = c["x"].shape
        Cw = c["hk"].shape[2]
        n = n if n_ is None else n_
        keep = [d(c["hk"] if hk is None else hk)] + [d(c[q]) for q in ("ln_w", "ln_b", "w_pred", "b_pred", "w_aemb", "bias_pos", "semb", "coef", "lo", "hi", "scale", "shift", "len")]
        self.t_dev = torch.tensor([t], dtype=torch.int32, device=dev) if t_dev is None else t_dev
        n_in = None if noise is None else d(c["noise"] if isinstance(noise, str) else noise)
        if state is None:
            self.x = d(c["x"] if x is None else x).clone()
            self.xbuf = torch.full((n, 2 * W + 1, Cw), SENT, device=dev)
            self.ring_t = d(c["ring"]).clone()
            self.act = torch.full((n, A), SENT, device=dev)
            self.bad_t = torch.full((n,), 0 if i >= 0 else 99, dtype=torch.int32, device=dev)
        else:
            self.x, self.xbuf, self.ring_t, self.act, self.bad_t = state
        self.no = torch.full((n, W, A), SENT, device=dev) if want_noise else None
        ptr = lambda v: None if v is None else v.data_ptr()
        self.rc = capi.load().d3il_beso_step(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), float(c["eps"]), *(ptr(q) for q in keep[3:9]), float(c["sigma_max"]), float(c["c_in0"]),
                                             *(ptr(q) for q in keep[9:]), int(seed), int(env_offset), ptr(self.t_dev), ptr(n_in), ptr(self.x), ptr(self.xbuf),
                                             ptr(self.ring_t) if W > 1 else None, ptr(self.act), ptr(self.bad_t), ptr(self.no), n, Cw if C_ is None else C_,
                                             A if A_ is None else A_, W if W_ is None else W_, c["S"] if S_ is None else S_, i, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        self.keep = keep + [n_in]
        self.state = (self.x, self.xbuf, self.ring_t, self.act, self.bad_t)
        self.x_out, self.buf, self.ring, self.actions, self.bad = self.x.cpu().numpy(), self.xbuf.cpu().numpy(), self.ring_t.cpu().numpy(), self.act.cpu().numpy(), self.bad_t.cpu().numpy()
        self.noise_out = None if self.no is None else self.no.cpu().numpy()


_FULL = {}


def full_case(dev, W, Cw, A, i):
    """(case, f64 result, launch) of the 257-environment problem of this (W, C, A, i): computed once, shared, left unchanged."""
    if (W, Cw, A, i) not in _FULL:
        c = make_case(257, W, Cw, A, seed=Cw * 10 + A)
        _FULL[W, Cw, A, i] = (c, step64(c, i), Launch(dev, c, i))
    return _FULL[W, Cw, A, i]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_against_f64(dev, c, ref, out, i):
    """One launch against the f64 restatement of ITS case: x', the token rows, a_new (the ring) and the actions within 4 x the deviation of torch's own f32 chain on
    the same device for the same case; plus what the launch must and must not write."""
    n, W, A = c["x"].shape
    Cw, last = c["hk"].shape[2], i == c["S"] - 1
    t_x, t_tok, t_new, t_act = torch_f32(dev, c, i)
    e_x, e_tok = float(np.abs(t_x - ref["xp"]).max()), float(np.abs(t_tok - ref["tok"]).max())
    assert out.rc == 0 and (out.bad == 0).all()
    tok = out.buf[:, 2::2]
    pad = ~ref["valid"]
    assert W == 1 or pad.any()
    if not last:
        k_x, k_tok = float(np.abs(out.x_out - ref["xp"]).max()), float(np.abs(tok - ref["tok"]).max())
        print("n %d W %d C %d A %d i %d: |x' - f64| kernel %.3e torch f32 %.3e (%.2f x); |token - f64| kernel %.3e torch f32 %.3e (%.2f x)" % (
            n, W, Cw, A, i, k_x, e_x, k_x / e_x if e_x else 0.0, k_tok, e_tok, k_tok / e_tok))
        assert k_x <= 4 * e_x and k_tok <= 4 * e_tok
        assert np.array_equal(out.buf[:, 0], np.broadcast_to(c["semb"][i + 1], (n, Cw)))      # the sigma token of the NEXT sampling step
        assert (out.buf[:, 1::2] == SENT).all() and (out.actions == SENT).all()                 # the state tokens and the action are not this launch's
        assert np.array_equal(out.ring, c["ring"])                                              # nor is the ring
        assert (out.x_out[pad] == 0.0).all() and np.array_equal(tok[pad], np.broadcast_to(c["bias_pos"][None], tok.shape)[pad])
        if i < 0:
            # the first iterate bit for bit: ring entries as they are, sigma_max * noise as the f32 product; one draw per environment, recorded at j = 0
            want = first_iterate(c, np.float32(c["sigma_max"]) * c["noise"][:, 0])
            assert np.array_equal(bits(out.x_out), bits(want))
            assert np.array_equal(out.noise_out[:, 0], c["noise"][:, 0]) and (out.noise_out[:, 1:] == 0.0).all()
        else:
            assert np.array_equal(out.noise_out, c["noise"])
    else:
        e_act, e_new = float(np.abs(t_act - ref["actions"]).max()), float(np.abs(t_new - ref["a_new"]).max())
        k_act = float(np.abs(out.actions - ref["actions"]).max())
        k_new = float(np.abs(out.ring[:, -1] - ref["a_new"]).max()) if W > 1 else 0.0
        print("n %d W %d C %d A %d i %d: |action - f64| kernel %.3e torch f32 %.3e (%.2f x); |a_new - f64| kernel %.3e torch f32 %.3e" % (
            n, W, Cw, A, i, k_act, e_act, k_act / e_act, k_new, e_new))
        assert k_act <= 4 * e_act and k_new <= 4 * e_new
        assert np.array_equal(out.x_out, c["x"]) and (out.buf == SENT).all()                  # the last step writes the action and the ring only
        assert (out.noise_out == 0.0).all()                                                    # and draws nothing
        if W > 1:
            assert np.array_equal(bits(out.ring[:, :-1]), bits(c["ring"][:, 1:]))             # the older entries move down by one, bit for bit
        pre = ref["xp"][np.arange(n), c["len"] - 1]
        assert 0.2 < float(np.mean((pre > c["lo"] + 1e-4) & (pre < c["hi"] - 1e-4))) < 1.0      # the clamp is exercised, and is not all there is


@pytest.mark.parametrize("Cw", [72, 120])
@pytest.mark.parametrize("A", [2, 3, 8])
@pytest.mark.parametrize("W", [1, 5])
def test_step_equals_the_f64_restatement(dev, W, A, Cw):
    """The 257-environment launch within 4 x the deviation torch's own f32 chain shows against f64 on the same device for the same 257 environments.  The launches of
    1 / 63 / 64 / 65 environments run the first rows of that case and must give those rows of the 257 launch BIT FOR BIT - x', every token row, the ring, the action,
    the noise, the flag: an environment's result does not depend on which wave, workgroup or pass serves it."""
    for i in (-1, 0, MID, S - 1):
        c, ref, full = full_case(dev, W, Cw, A, i)
        check_against_f64(dev, c, ref, full, i)
        for n in (1, 63, 64, 65):
            out = Launch(dev, first_rows(c, n), i)
            assert out.rc == 0
            for name in ("x_out", "buf", "ring", "actions", "noise_out", "bad"):
                assert np.array_equal(bits(getattr(out, name)), bits(getattr(full, name)[:n])), (n, i, name)


@pytest.mark.parametrize("Cw", [32, 100, 128])
def test_run_time_width_instantiation(dev, Cw):
    for i in (-1, 0, MID, S - 1):
        c, ref, full = full_case(dev, 5, Cw, 8, i)
        check_against_f64(dev, c, ref, full, i)


def test_three_passes_behind_the_grid_cap(dev):
    """8200 environments: the grid is capped at 1024 workgroups = 4096 waves, so every wave makes three passes, the third with 8 live waves.  Same bar, on this case;
    and the first 257 environments equal a 257-environment launch bit for bit."""
    for i in (MID, S - 1):
        c = make_case(8200, 2, 72, 2, seed=31)
        out = Launch(dev, c, i)
        check_against_f64(dev, c, step64(c, i), out, i)
        small = Launch(dev, first_rows(c, 257), i)
        for name in ("x_out", "buf", "ring", "actions"):
            assert np.array_equal(bits(getattr(small, name)), bits(getattr(out, name)[:257])), (i, name)


def test_clamp_edges_are_exact(dev):
    """The last step's x' is (nearly) den = c_out net + c_skip x: the head's bias pushes it far above the upper bound on component 0 and far below the lower one on
    component 1: a_new (the ring's newest entry) and, with unit output scaling, the action come out as the bounds, bit for bit; the others stay strictly inside."""
    c = make_case(65, 5, 120, 8, seed=3)
    c["b_pred"][0], c["b_pred"][1] = 50000.0, -50000.0
    c["x"] *= 0.15
    c["scale"][:], c["shift"][:] = 1.0, 0.0
    ref = step64(c, S - 1)
    out = Launch(dev, c, S - 1)
    assert out.rc == 0 and (out.bad == 0).all()
    assert abs(ref["xp"][:, :, 0]).max() > 100 * c["hi"][0]
    for got in (out.actions, out.ring[:, -1]):
        assert (got[:, 0] == c["hi"][0]).all() and (got[:, 1] == c["lo"][1]).all()
        assert (got[:, 2:] > c["lo"][2:]).all() and (got[:, 2:] < c["hi"][2:]).all() and float(np.abs(got[:, 2:] - ref["a_new"][:, 2:]).max()) < 1e-5


def test_the_last_step_ignores_its_noise(dev):
    c = make_case(65, 5, 120, 8, seed=4)
    a = Launch(dev, c, S - 1, noise=np.zeros_like(c["noise"]))
    b = Launch(dev, c, S - 1, noise=np.full_like(c["noise"], 1e30))
    d = Launch(dev, c, S - 1, noise=None)
    assert np.array_equal(bits(a.actions), bits(b.actions)) and np.array_equal(bits(a.actions), bits(d.actions)) and np.array_equal(bits(a.ring), bits(d.ring))
    assert np.isfinite(a.actions).all() and (d.noise_out == 0.0).all()


CHAIN_S = 6


def run_chain(dev, c, hks, poison=None):
    """Init launch, then steps 0 .. S - 1 on one state, hidden rows hks[i]; ``poison`` = (i, env, position, element, value) is put into that launch's rows.
    Returns the launches by step index."""
    out = {-1: Launch(dev, c, -1)}
    state = out[-1].state
    for i in range(c["S"]):
        hk = hks[i]
        if poison is not None and poison[0] == i:
            hk = hk.copy()
            hk[poison[1], poison[2], poison[3]] = poison[4]
        out[i] = Launch(dev, c, i, hk=hk, state=state)
    return out


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("when", [0, 3])
def test_nonfinite_rows_mark_their_environment_and_leave_the_neighbours_alone(dev, when, value):
    """A NaN / an Inf in one environment's hidden rows at the first / at a middle sampling step: that environment's action and pushed ring entry are NaN, ``bad`` is
    sticky across the launches that follow (their hidden rows are clean), every other environment is bit-equal to a clean chain; a NaN at a PADDED position marks
    nothing; the next init launch clears the flag, and the NaN ring entry marks the environment again once its window reads it."""
    n, W, Cw, A, s = 65, 5, 120, 8, CHAIN_S
    c = make_case(n, W, Cw, A, seed=9, s=s)
    rng = np.random.default_rng(19)
    hks = {i: (rng.normal(size=(n, W, Cw)) * 1.7 + 0.3).astype(np.float32) for i in range(s)}
    e = 40
    assert c["len"][e] >= 2 and c["len"][7] < W
    clean = run_chain(dev, c, hks)
    dirty = run_chain(dev, c, hks, poison=(when, e, 0, 17, value))
    others = np.arange(n) != e
    assert clean[-1].bad.tolist() == [0] * n and (clean[s - 1].bad == 0).all() and np.isfinite(clean[s - 1].actions).all()
    for i in range(s):
        assert (dirty[i].bad[others] == 0).all() and int(dirty[i].bad[e]) == (1 if i >= when else 0), i
    last, mid = s - 1, s - 2
    assert np.isnan(dirty[last].actions[e]).all() and np.isnan(dirty[last].ring[e, -1]).all()
    assert np.array_equal(bits(dirty[last].actions[others]), bits(clean[last].actions[others]))
    assert np.array_equal(bits(dirty[last].ring[others]), bits(clean[last].ring[others]))
    assert np.array_equal(bits(dirty[mid].x_out[others]), bits(clean[mid].x_out[others]))
    assert np.array_equal(bits(dirty[mid].buf[others]), bits(clean[mid].buf[others]))
    padded = run_chain(dev, c, hks, poison=(when, 7, W - 1, 3, value))
    assert (padded[last].bad == 0).all() and np.array_equal(bits(padded[last].actions), bits(clean[last].actions))
    # the init launch clears the flag - and sets it again where the window reads the NaN entry of the ring (len >= 2: the newest ring entry is read)
    again = Launch(dev, c, -1, state=dirty[last].state)
    assert (again.bad[others] == 0).all() and int(again.bad[e]) == 1
    fresh = dict(c, len=np.ones_like(c["len"]))
    assert (Launch(dev, fresh, -1, state=dirty[last].state).bad == 0).all()      # a restarted lane does not read its ring


def test_a_bad_environment_raises_solver_fail_in_its_stacking_lane_only(dev):
    """The kernel's NaN action, used as the Sim uses a policy output (simulation/_rollout.py joint_rollout), for one env step of Stacking."""
    from d3il_amd.envs.stacking import CubeStackingVecEnv, load_test_contexts
    n = 6
    c = make_case(n, 5, 120, 8, seed=10)
    c["scale"][:], c["shift"][:] = 0.003, 0.0
    hk = c["hk"].copy()
    hk[2, 0, 5] = np.nan
    out = Launch(dev, c, S - 1, hk=hk)
    assert out.bad.tolist() == [0, 0, 1, 0, 0, 0] and np.isnan(out.actions[2]).all() and np.isfinite(np.delete(out.actions, 2, axis=0)).all()
    env = CubeStackingVecEnv(n, device=dev, render=False, max_steps_per_episode=12)
    try:
        env.start()
        env.reset(random=False, context=load_test_contexts()[:n])
        rs = env.robot_state()
        a = out.act.to(torch.float64)
        env.step(torch.cat((a[:, :7] + rs[:, :7], a[:, 7:8]), dim=1).contiguous())
        torch.cuda.synchronize()
        fail = (env.flags[:n] & SOLVER_FAIL) != 0
        assert fail.tolist() == [r == 2 for r in range(n)]
    finally:
        env.close()


def test_philox_stream(dev):
    from d3il_amd import policies as P
    seed, t, i, n, W, A = 0x1234567890ABCDEF, 7, 4, 257, 5, 8
    c = make_case(n, W, 72, A, seed=11)
    whole = Launch(dev, c, i, noise=None, seed=seed, t=t)
    want = P.beso_normals(seed, 0, n, t, i + 1, W, A)
    # the yardstick: torch's f32 evaluation of the same Box-Muller formula on the same words, on the device
    w = torch.as_tensor(P.beso_words(seed, 0, n, t, i + 1, W).astype(np.int64)).to(dev)
    u1 = ((w[..., 0::2] >> 8) + 1).float() * (2.0 ** -24)
    u2 = (w[..., 1::2] >> 8).float() * (2.0 ** -24)
    rad, ang = torch.sqrt(-2.0 * torch.log(u1)), 6.283185307179586 * u2
    z32 = torch.stack((rad * torch.cos(ang), rad * torch.sin(ang)), dim=-1).reshape(n, W, 8)[:, :, :A].double().cpu().numpy()
    e32, e_k = float(np.abs(z32 - want).max()), float(np.abs(whole.noise_out - want).max())
    print("Box-Muller against f64: kernel %.3e, torch f32 %.3e; largest |normal| %.2f" % (e_k, e32, float(np.abs(want).max())))
    assert e_k <= 4 * e32 and np.isfinite(whole.noise_out).all()
    # the launch used what it reports: against a launch that gets the same numbers handed in
    fed = Launch(dev, c, i, noise=whole.noise_out)
    assert np.array_equal(fed.x_out, whole.x_out) and np.array_equal(fed.buf, whole.buf)
    # a launch on environments 100 .. 163 with env_offset 100 = the slice of the 257-environment launch
    sl = slice(100, 164)
    part_case = dict(c, hk=c["hk"][sl], x=c["x"][sl], ring=c["ring"][sl], len=c["len"][sl], noise=c["noise"][sl])
    part = Launch(dev, part_case, i, noise=None, seed=seed, env_offset=100, t=t)
    assert np.array_equal(part.noise_out, whole.noise_out[sl]) and np.array_equal(part.x_out, whole.x_out[sl]) and np.array_equal(part.buf, whole.buf[sl])
    # the init mode: draw 0, position 0, one per environment - at len - 1 of x' times sigma_max; and its env_offset slice; A = 3 takes the first three components
    init = Launch(dev, c, -1, noise=None, seed=seed, t=t)
    z0 = P.beso_normals(seed, 0, n, t, 0, W, A)[:, 0]
    assert float(np.abs(init.noise_out[:, 0] - z0).max()) <= 4 * e32 and (init.noise_out[:, 1:] == 0.0).all() and not np.array_equal(init.noise_out[:, 0], whole.noise_out[:, 0])
    assert np.array_equal(bits(init.x_out[np.arange(n), c["len"] - 1]), bits(np.float32(c["sigma_max"]) * init.noise_out[:, 0]))
    part0 = Launch(dev, part_case, -1, noise=None, seed=seed, env_offset=100, t=t)
    assert np.array_equal(part0.noise_out, init.noise_out[sl]) and np.array_equal(part0.x_out, init.x_out[sl])
    c3 = make_case(n, W, 72, 3, seed=11)
    three = Launch(dev, c3, i, noise=None, seed=seed, t=t)
    assert np.array_equal(three.noise_out, whole.noise_out[:, :, :3])
    # the device step word: advanced between two launches -> other numbers; the same word -> the same bits
    word = torch.tensor([t], dtype=torch.int32, device=dev)
    a = Launch(dev, c, i, noise=None, seed=seed, t_dev=word)
    b = Launch(dev, c, i, noise=None, seed=seed, t_dev=word)
    word.add_(1)
    d = Launch(dev, c, i, noise=None, seed=seed, t_dev=word)
    assert np.array_equal(a.noise_out, whole.noise_out) and np.array_equal(a.noise_out, b.noise_out) and np.array_equal(a.x_out, b.x_out)
    assert not np.array_equal(d.noise_out, a.noise_out)
    assert float(np.abs(d.noise_out - P.beso_normals(seed, 0, n, t + 1, i + 1, W, A)).max()) <= 4 * e32


def test_unsupported_shapes_are_refused_before_any_launch(dev):
    c = make_case(4, 5, 120, 3, seed=12)
    for kw in (dict(C_=130), dict(C_=122), dict(A_=9), dict(A_=0), dict(W_=17), dict(W_=0), dict(S_=255), dict(S_=0)):
        out = Launch(dev, c, 3 if kw.get("S_") != 0 else -1, **kw)
        assert out.rc == -5, kw
        assert (out.buf == SENT).all() and (out.actions == SENT).all() and np.array_equal(out.x_out, c["x"]) and (out.noise_out == SENT).all() and np.array_equal(out.ring, c["ring"]), kw
    ok = Launch(dev, c, 3)
    assert ok.rc == 0 and (ok.buf[:, 0] != SENT).all()
