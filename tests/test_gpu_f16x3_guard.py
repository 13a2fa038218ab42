"""Range / NaN guard of the split-f16 policy kernels on the GPU (csrc/policy_f16x3.h GUARD instantiations; include/d3il_rollout.h d3il_f16x3_set_guard;
policies.RangeGuard; the Sims' policy_range_guard).  Every case runs with the guard off first: that output is what "bit-equal" refers to.  Shapes are the
smallest that reach the padding paths: 37 rows = one workgroup of four waves with a partly filled third wave (rows 32 .. 36 live, 11 lanes re-reading row 36)
and a dead fourth one; (B, T) = (3, 11) and (5, 16) = both attention instantiations with dead waves, and padding tokens for T = 11."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS = 37
SOLVER_FAIL = 1 << 16


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def blk(dev):
    from d3il_amd.policies import _Block
    torch.manual_seed(5)
    b = _Block(120, 6, 16).eval()
    for p in b.parameters():
        p.requires_grad_(False)
    return b.to(dev)


@pytest.fixture()
def guard(dev, monkeypatch):
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_RANGE_GUARD", raising=False)
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    assert P.range_guard() is None
    g = P.RangeGuard(dev)
    yield g
    g.disable()
    assert P.range_guard() is None


def _counts(g):
    r = g.read()
    return (r["clipped"], r["nonfinite"], r["launches"])


def _off_then_on(g, fn):
    """fn() with the guard off, then on: (output off, output on, counters of the guarded run)."""
    off = fn()
    torch.cuda.synchronize()
    g.reset()
    with g:
        on = fn()
        c = _counts(g)
    return off, on, c


def _bad_rows(out):
    return set(torch.nonzero(~torch.isfinite(out.reshape(-1, out.shape[-1])).all(dim=1)).reshape(-1).tolist())


def _any_bad_rows(out):
    return set(torch.nonzero((~torch.isfinite(out.reshape(-1, out.shape[-1]))).any(dim=1)).reshape(-1).tolist())


def _linear(dev, x, W, bias, resid, ln, f32=False):
    from d3il_amd import capi, policies as P
    L = capi.load()
    N = W.shape[0]
    out = torch.full((x.shape[0], N), 12345.0, device=dev)
    wp = P.pack_linear120_weights(W) if f32 else P.pack_linear120_weights_f16x3(W)
    fn = L.d3il_linear120_f32 if f32 else L.d3il_linear120_f16x3
    lw, lb, eps = (ln[0].data_ptr(), ln[1].data_ptr(), float(ln[2])) if ln is not None else (None, None, 0.0)
    capi.check(fn(x.data_ptr(), lw, lb, eps, wp.data_ptr(), bias.data_ptr(), None if resid is None else resid.data_ptr(), out.data_ptr(), x.shape[0], N,
                  torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N", [360, 120])
def test_linear_without_layernorm_counts_exactly(dev, blk, guard, N):
    a = blk.attn
    if N == 360:
        W, bias, resid = torch.cat((a.query.weight, a.key.weight, a.value.weight), 0).contiguous(), torch.cat((a.query.bias, a.key.bias, a.value.bias), 0).contiguous(), None
    else:
        W, bias = a.proj.weight.contiguous(), a.proj.bias.contiguous()
        resid = torch.randn(ROWS, 120, generator=torch.Generator().manual_seed(2)).to(dev)
    x = torch.randn(ROWS, 120, generator=torch.Generator().manual_seed(1)).to(dev)
    x[3, 7], x[36, 119], x[20, 0], x[21, 5] = 7e4, -1e5, float("nan"), float("inf")      # row 36: the row the padding lanes re-read
    off, on, c = _off_then_on(guard, lambda: _linear(dev, x, W, bias, resid, None))
    assert c == (2, 2, 1), c
    assert _bad_rows(on) == {20, 21} == _any_bad_rows(on)                                   # non-finite in EVERY column, and no other row
    keep = [r for r in range(ROWS) if r not in (20, 21)]
    assert torch.equal(on[keep], off[keep]) and torch.isfinite(off[[3, 36]]).all()
    print("unguarded linear N = %d, NaN row 20 / Inf row 21: all finite = %s / %s" % (N, bool(torch.isfinite(off[20]).all()), bool(torch.isfinite(off[21]).all())))
    assert _any_bad_rows(_linear(dev, x, W, bias, resid, None, f32=True)) == {20, 21}      # the f32 kernel on the same input
    # a second guarded launch adds to the same counters; the reserved word stays untouched
    with guard:
        _linear(dev, x, W, bias, resid, None)
        assert _counts(guard) == (4, 4, 2) and int(guard.counts[3]) == 0


def _ln64(x, w, b, eps):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def test_linear_with_layernorm_counts_the_rows_an_f64_layernorm_puts_out_of_range(dev, blk, guard):
    a = blk.attn
    W, bias = torch.cat((a.query.weight, a.key.weight, a.value.weight), 0).contiguous(), torch.cat((a.query.bias, a.key.bias, a.value.bias), 0).contiguous()
    x = (torch.randn(ROWS, 120, generator=torch.Generator().manual_seed(7)) * 2 + 0.3).to(dev)      # 33 rows out of range (row 36, the one the padding lanes re-read, among them), 4 in range
    lw, lb = blk.ln1.weight.clone(), blk.ln1.bias.clone()
    lw[11] = 1e6
    op = _ln64(x, lw, lb, blk.ln1.eps).abs()
    must = (op > 65504.0 * (1 + 1e-4)).any(dim=1)
    must_not = (op < 65504.0 * (1 - 1e-4)).all(dim=1)
    # the band +-1e-4 is ~100 x the f32-against-f64 difference of a LayerNorm output (a few ulp = 1e-6 relative): no row of this input is left undecided
    assert bool((must | must_not).all()) and int(must.sum()) > 0 and int(must_not.sum()) > 0
    off, on, c = _off_then_on(guard, lambda: _linear(dev, x, W, bias, None, (lw, lb, blk.ln1.eps)))
    assert c == (int(must.sum()), 0, 1), (c, int(must.sum()))
    assert torch.equal(on, off) and torch.isfinite(on).all()


def _mlp(dev, blk, x, b1=None):
    from d3il_amd import capi
    L = capi.load()
    blk.ensure_packed()
    fc1, fc2 = blk.mlp[0], blk.mlp[2]
    b1 = fc1.bias if b1 is None else b1
    out = torch.full_like(x, 12345.0)
    capi.check(L.d3il_mlp_ln_gelu_residual_f16x3(x.data_ptr(), blk.ln2.weight.data_ptr(), blk.ln2.bias.data_ptr(), float(blk.ln2.eps), x.data_ptr(), blk._hp_mlp.data_ptr(),
                                                 b1.data_ptr(), fc2.bias.data_ptr(), out.data_ptr(), x.shape[0], 120, 480, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return out


def test_mlp_counts_live_rows_once(dev, blk, guard):
    x = torch.randn(ROWS, 120, generator=torch.Generator().manual_seed(7)).to(dev)
    # clean O(1) input: nothing but the launch is counted (the two empty half stages of the pipeline make no marks)
    off, on, c = _off_then_on(guard, lambda: _mlp(dev, blk, x))
    assert c == (0, 0, 1), c
    assert torch.equal(on, off) and torch.isfinite(on).all()
    # GELU output 5 of every row = 1e5: 37 live rows, not the 48 lanes-rows of three waves
    b1 = blk.mlp[0].bias.clone()
    b1[5] = 1e5
    off, on, c = _off_then_on(guard, lambda: _mlp(dev, blk, x, b1))
    assert c == (ROWS, 0, 1), c
    assert torch.equal(on, off) and torch.isfinite(on).all()
    # a NaN input element: its row is NaN in all 120 columns, every other row is untouched
    xn = x.clone()
    xn[9, 0] = float("nan")
    off, on, c = _off_then_on(guard, lambda: _mlp(dev, blk, xn))
    assert c == (0, 1, 1), c
    assert _bad_rows(on) == {9} == _any_bad_rows(on)
    keep = [r for r in range(ROWS) if r != 9]
    assert torch.equal(on[keep], off[keep])


def _attn(dev, blk, x, b_qkv=None):
    from d3il_amd import capi
    L = capi.load()
    blk.ensure_packed()
    B, T, C = x.shape
    out = torch.full_like(x, 12345.0)
    b_qkv = blk._b_qkv if b_qkv is None else b_qkv
    capi.check(L.d3il_attn_half_f16x3(x.data_ptr(), blk.ln1.weight.data_ptr(), blk.ln1.bias.data_ptr(), float(blk.ln1.eps), blk._hp_attn.data_ptr(), b_qkv.data_ptr(),
                                      blk.attn.proj.bias.data_ptr(), out.data_ptr(), B, T, 6, C, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,T", [(3, 11), (5, 16)])
def test_attention_half_marks_the_rows_a_nan_token_reaches(dev, blk, guard, monkeypatch, B, T):
    x = torch.randn(B, T, 120, generator=torch.Generator().manual_seed(B * 100 + T)).to(dev)
    off, on, c = _off_then_on(guard, lambda: _attn(dev, blk, x))
    assert c == (0, 0, 1) and torch.equal(on, off) and torch.isfinite(on).all()
    xn = x.clone()
    xn[1, 4, 0] = float("nan")
    off, on, c = _off_then_on(guard, lambda: _attn(dev, blk, xn))
    expect = {T + t for t in range(4, T)}                                                   # tokens 4 .. T - 1 of sequence 1: token 4 at both sites (once), the later ones through its key / value rows
    assert c == (0, T - 4, 1), c
    assert _bad_rows(on) == expect == _any_bad_rows(on)
    keep = [r for r in range(B * T) if r not in expect]
    assert torch.equal(on.reshape(B * T, 120)[keep], off.reshape(B * T, 120)[keep])
    # the block's three-kernel f32 path: the same rows (the MLP behind the attention half works row by row)
    monkeypatch.setenv("D3IL_POLICY_GEMM", "f32")
    with torch.no_grad():
        y32 = blk(xn)
    monkeypatch.delenv("D3IL_POLICY_GEMM")
    assert _any_bad_rows(y32) == expect
    # a value bias of 1e5: attention output 3 of every token is 1e5 - every live token counts, no padding token and no dead wave does
    bq = blk._b_qkv.clone()
    bq[240 + 3] = 1e5
    off, on, c = _off_then_on(guard, lambda: _attn(dev, blk, x, bq))
    assert c == (B * T, 0, 1), c
    assert torch.equal(on, off) and torch.isfinite(on).all()


def _beso(dev, seed=11):
    import bench
    pol = bench._random_beso(dev)
    pol.use_graph = False
    gen = torch.Generator(device=dev).manual_seed(seed)
    pol.noise_fn = lambda shape: torch.randn(shape, generator=gen, device=dev)
    return pol


def _two_calls(dev, obs):
    pol = _beso(dev)
    return torch.stack([pol.predict_batch(obs).clone(), pol.predict_batch(obs + 0.01).clone()])


def test_policy_actions_and_report(dev, guard, monkeypatch):
    from d3il_amd import policies as P
    from d3il_amd.envs.stacking import CubeStackingVecEnv, load_test_contexts
    n = 6
    obs = torch.randn(n, 20, generator=torch.Generator().manual_seed(3)).to(dev)
    obs_nan = obs.clone()
    obs_nan[2, 4] = float("nan")
    clean_off = _two_calls(dev, obs)
    guard.reset()
    with guard:
        clean_on = _two_calls(dev, obs)
        pol = _beso(dev)
        pol.predict_batch(obs)
        rep = pol.range_report()
        nan_on = _two_calls(dev, obs_nan)
        assert guard.read()["nonfinite"] > 0
    assert torch.equal(clean_on, clean_off) and torch.isfinite(clean_on).all()
    assert rep["clipped"] == 0 and rep["nonfinite"] == 0 and rep["launches"] > 0 and rep["weights_out_of_range"] == 0, rep
    others = [r for r in range(n) if r != 2]
    assert not torch.isfinite(nan_on[:, 2]).any()
    assert torch.equal(nan_on[:, others], clean_on[:, others])
    # the f32 kernels: the same pattern
    monkeypatch.setenv("D3IL_POLICY_GEMM", "f32")
    clean32, nan32 = _two_calls(dev, obs), _two_calls(dev, obs_nan)
    monkeypatch.delenv("D3IL_POLICY_GEMM")
    assert not torch.isfinite(nan32[:, 2]).any() and torch.equal(nan32[:, others], clean32[:, others]) and torch.isfinite(clean32).all()
    # what the UNGUARDED split-f16 path does with the same input (recorded in DESIGN, not asserted: it is the hole the guard closes)
    nan_off = _two_calls(dev, obs_nan)
    print("unguarded f16x3, NaN in observation row 2: action row 2 =", nan_off[:, 2].tolist(), "other rows equal to the clean run:", torch.equal(nan_off[:, others], clean_off[:, others]))
    # the step kernel catches the guarded policy's NaN action: lane 2 and only lane 2
    env = CubeStackingVecEnv(n, device=dev, render=False, max_steps_per_episode=12)
    try:
        env.start()
        env.reset(random=False, context=load_test_contexts()[:n])
        rs = env.robot_state()
        out = nan_on[0].to(torch.float64)
        env.step(torch.cat((out[:, :7] + rs[:, :7], out[:, 7:8]), dim=1).contiguous())       # the Sim's action (simulation/_rollout.py joint_rollout)
        torch.cuda.synchronize()
        fail = (env.flags[:n] & SOLVER_FAIL) != 0
        assert fail.tolist() == [r == 2 for r in range(n)]
    finally:
        env.close()


def test_captured_sampling_loop_is_captured_again_when_the_guard_changes(dev, guard, monkeypatch):
    import bench
    monkeypatch.setenv("D3IL_POLICY_GRAPH", "1")
    pol = bench._random_beso(dev)
    assert pol.use_graph
    obs = torch.randn(6, 20, generator=torch.Generator().manual_seed(4)).to(dev)
    for _ in range(5):                    # window 5: the fifth call has a full window and captures the sampling loop - guard off
        pol.predict_batch(obs)
    torch.cuda.synchronize()
    assert pol._graph is not None
    g_off = pol._graph
    guard.reset()
    with guard:
        pol.predict_batch(obs)
        first = guard.read()["launches"]
        assert first > 0 and pol._graph is not g_off          # the unguarded graph was not replayed while the guard read as enabled
        pol.predict_batch(obs)                                  # a replay of the guarded graph: 16 sampling steps x 6 blocks x (attention half + MLP)
        assert guard.read()["launches"] - first == 16 * 6 * 2
        g_on = pol._graph
    a = pol.predict_batch(obs)
    torch.cuda.synchronize()
    assert pol._graph is not g_on and torch.isfinite(a).all()
    assert guard.read()["launches"] == first + 16 * 6 * 2     # and the guarded graph is not replayed once the guard is off


def test_stacking_sim_reports_the_policy_range(dev, monkeypatch):
    import bench
    from d3il_amd import policies as P
    from d3il_amd.simulation.stacking_sim import Stacking_Sim
    monkeypatch.delenv("D3IL_POLICY_RANGE_GUARD", raising=False)
    res = {}
    for on in (False, True):
        sim = Stacking_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_contexts=5, n_trajectories_per_context=3, max_steps_per_episode=12, policy_range_guard=on)
        pol = bench._random_beso(dev)
        pol.use_graph = False
        gen = torch.Generator(device=dev).manual_seed(9)
        pol.noise_fn = lambda shape, gen=gen: torch.randn(shape, generator=gen, device=dev)
        tables = sim.test_agent(pol)
        res[on] = (tables, sim.last_rollout)
        assert P.range_guard() is None                          # the Sim switches its guard off again
    assert res[False][1]["policy_range"] is None
    rep = res[True][1]["policy_range"]
    assert rep["clipped"] == 0 and rep["nonfinite"] == 0 and rep["weights_out_of_range"] == 0 and rep["launches"] > 0, rep
    for k in (0, 1):
        assert torch.equal(res[True][0][k], res[False][0][k])
    for key in ("mode", "success", "mean_distance", "flags"):
        assert torch.equal(res[True][1][key], res[False][1][key]), key
