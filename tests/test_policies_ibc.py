"""policies.IBCPolicy on the CPU against the reference's own IBCAgent + EBMMLP + LangevinMCMCSampler: tests/golden/ref_ibc_agent.npz holds fixed-seed weights, a
scaler, banks for the three sources of randomness (start points, normals, the draw's uniform) and the reference rolled out batch-1 per environment TWICE - in f32 as
shipped and in f64 (tests/golden/gen_ibc_goldens.py, run where the reference is).  D / D_x / D_E = max |f32 - f64| of the reference's own actions / final samples /
energies are the yardsticks; the replay (the torch chain with the analytic gradient) must stay within 4 of them of the f64 tables and give the same picks on all 16
rows.  The device replay of the same fixture is tests/test_gpu_policies_ibc.py."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from d3il_amd import policies as P  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ibc_agent.npz"))
OBS, A, HIDDEN, LAYERS, S, ITER = (int(v) for v in G["ibc_cfg"])
K = 2 * ITER
D, DX, DE = (float(v) for v in G["ibc_D"])
NOISE_SCALE, CLIP, INIT_INFER, INIT, FINAL, POWER, SECOND = (float(v) for v in G["ibc_settings"])


def golden_sd(prefix="mlp."):
    return {prefix + k[len("ibc_sd__"):].replace("__", ".")[len("mlp."):]: torch.as_tensor(G[k]) for k in G.files if k.startswith("ibc_sd__")}


def golden_policy(dev, seed=0, **banks):
    sc = P.Scaler(G["ibc_x_mean"], G["ibc_x_std"], G["ibc_y_mean"], G["ibc_y_std"], G["ibc_y_bounds"], device=dev)
    net = P.ResidualMLP(OBS + A, HIDDEN, LAYERS, 1).to(dev)
    for p in net.parameters():
        p.requires_grad_(False)
    pol = P.IBCPolicy(net, sc, P.ibc_step_sizes(ITER, INIT_INFER, INIT, FINAL, POWER, SECOND), noise_scale=NOISE_SCALE, delta_action_clip=CLIP, samples=S, seed=seed,
                      bounds=G["ibc_y_bounds"], **banks)
    pol.load_reference_state_dict(golden_sd())
    return pol


class Banks:
    """x0_in / noise_in / u_in that replay the golden banks of step ``t`` ([N, T, ...] tables)."""

    def __init__(self):
        self.t = 0
        self.x0_in = lambda n: G["ibc_x0"][:n, self.t]
        self.noise_in = lambda n: np.moveaxis(G["ibc_noise"][:n, self.t], 1, 0)
        self.u_in = lambda n: G["ibc_u"][:n, self.t]

    def kw(self):
        return dict(x0_in=self.x0_in, noise_in=self.noise_in, u_in=self.u_in)


def replay(dev):
    """Worst deviations of the golden replay on ``dev`` from the f64 tables: (actions, final samples, energies, picks equal on all rows, policy)."""
    b = Banks()
    pol = golden_policy(dev, **b.kw())
    pol.record = True
    obs = G["ibc_obs"]
    wa = wx = we = 0.0
    same = True
    for t in range(obs.shape[1]):
        b.t = t
        a = pol.predict_batch(torch.as_tensor(obs[:, t], device=dev)).cpu().numpy().astype(np.float64)
        wa = max(wa, float(np.abs(a - G["ibc_ref64"][:, t]).max()))
        wx = max(wx, float(np.abs(pol.last_x.cpu().numpy().astype(np.float64) - G["ibc_x64"][:, t]).max()))
        we = max(we, float(np.abs(pol.last_energies.cpu().numpy().astype(np.float64) - G["ibc_e64"][:, t]).max()))
        same = same and np.array_equal(pol.last_picks.cpu().numpy().astype(np.int64), G["ibc_picks64"][:, t])
    return wa, wx, we, same, pol


def test_policy_rows_equal_reference_predict():
    assert float(np.abs(G["ibc_ref32"] - G["ibc_ref64"]).max()) == D and G["ibc_ref64"].shape == (4, 4, A) and np.array_equal(G["ibc_picks32"], G["ibc_picks64"])
    edge = np.abs(G["ibc_cdf64"] - G["ibc_u"][:, :, None].astype(np.float64)).min()
    assert edge >= 1e-4      # every golden pick is decided
    wa, wx, we, same, pol = replay("cpu")
    print("golden replay (cpu): actions %.3e = %.2f D, final samples %.3e = %.2f D_x, energies %.3e = %.2f D_E (D %.3e, D_x %.3e, D_E %.3e)" % (wa, wa / D, wx, wx / DX, we, we / DE, D, DX, DE))
    assert same
    assert wa <= 4 * D and wx <= 4 * DX and we <= 4 * DE
    assert int(pol._t) == 4


def test_step_size_table_is_the_references_schedule():
    assert P.ibc_step_sizes(ITER, INIT_INFER, INIT, FINAL, POWER, SECOND) == G["ibc_steps"].tolist() and len(G["ibc_steps"]) == K
    assert P.ibc_step_sizes(7, INIT_INFER, INIT, FINAL, POWER, SECOND) == G["ibc_steps7"].tolist()
    one = P.ibc_step_sizes(ITER, INIT_INFER, INIT, FINAL, POWER, SECOND, second=False)
    assert one == G["ibc_steps"].tolist()[:ITER]
    assert one[0] == INIT_INFER and one[1] < INIT and one[-1] == FINAL      # the schedule starts from sampler_stepsize_init, not from the _infer value
    pol = golden_policy("cpu")
    assert np.array_equal(pol.coef.numpy(), np.stack([(G["ibc_steps"] * 0.5).astype(np.float32), G["ibc_steps"].astype(np.float32)], axis=1))


@pytest.mark.parametrize("hidden,blocks,A_", [(128, 3, 2), (256, 4, 8), (128, 0, 8), (256, 1, 2)])
def test_analytic_gradient_equals_autograd_in_f64(hidden, blocks, A_):
    F = torch.nn.functional
    torch.manual_seed(hidden + blocks)
    obs = 20
    net = P.ResidualMLP(obs + A_, hidden, 2 * blocks, 1).double()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.6)
    rows = torch.randn(40, obs + A_, dtype=torch.float64) * 1.5
    rows[0] *= 20.0      # pre-activations beyond 20: the softplus threshold
    x = rows.clone().requires_grad_(True)
    lin_in, blks, lin_out = net._parts()
    h = lin_in(x)
    assert float(h.detach().max()) > 20.0
    for l1, l2 in blks:
        h = h + l2(F.mish(l1(F.mish(h))))
    e = lin_out(h)[:, 0]
    g, = torch.autograd.grad(e.sum(), x)
    with torch.no_grad():
        e2, g2 = P.resmlp_energy_and_grad(net, rows, obs)
    assert float((e2 - e).abs().max()) <= 1e-10 * float(e.abs().max())
    assert float((g2 - g[:, obs:]).abs().max()) <= 1e-10 * float(g[:, obs:].abs().max())


# ---- duck-typed reference agents (class names as in the reference: matches() goes by them)
class LangevinMCMCSampler:
    def __init__(self, poly=True, iters=ITER, second=True):
        self.noise_scale_infer, self.inference_samples, self.inference_iterations = NOISE_SCALE, S, iters
        self.sampler_stepsize_init, self.sampler_stepsize_init_infer, self.second_inference_stepsize_init = INIT, INIT_INFER, SECOND
        self.sampler_stepsize_final, self.sampler_stepsize_power, self.delta_action_clip, self.second_infer = FINAL, POWER, CLIP, second
        self._use_polynomial_rate = poly
        if poly:
            self.infer_schedule = object()
        else:
            self._schedule = object()
        self.bounds = G["ibc_y_bounds"]


class CorrectLangevinMCMCSampler(LangevinMCMCSampler):
    pass


class DerivativeFreeOptimizer:
    bounds = G["ibc_y_bounds"]


class _Block(torch.nn.Module):
    def __init__(self, h, act="Mish", use_norm=False):
        super().__init__()
        self.l1, self.l2 = torch.nn.Linear(h, h), torch.nn.Linear(h, h)
        self.act, self.use_norm = getattr(torch.nn, act)(), use_norm


class _Net(torch.nn.Module):
    def __init__(self, act="Mish", use_norm=False, spectral=False):
        super().__init__()
        first = torch.nn.Linear(OBS + A, HIDDEN)
        self.layers = torch.nn.ModuleList([torch.nn.utils.spectral_norm(first) if spectral else first] + [_Block(HIDDEN, act, use_norm) for _ in range(LAYERS // 2)]
                                          + [torch.nn.Linear(HIDDEN, 1)])


class EBMMLP(torch.nn.Module):
    def __init__(self, **kw):
        super().__init__()
        self.mlp = _Net(**kw)


class EBMConvMLP(EBMMLP):
    pass


def fake_agent(sampler=None, model=None, goal=False, ema=False):
    ag = types.SimpleNamespace(sampler=sampler or LangevinMCMCSampler(), model=model or EBMMLP(), goal_conditioning=goal, use_ema=ema,
                               scaler=types.SimpleNamespace(x_mean=torch.as_tensor(G["ibc_x_mean"]), x_std=torch.as_tensor(G["ibc_x_std"]), y_mean=torch.as_tensor(G["ibc_y_mean"]),
                                                            y_std=torch.as_tensor(G["ibc_y_std"]), y_bounds=G["ibc_y_bounds"]),
                               predict=lambda s: np.zeros(A))
    if not spectral_first(ag.model):
        ag.model.load_state_dict(golden_sd())
    return ag


def spectral_first(model):
    return hasattr(model.mlp.layers[0], "weight_orig")


def test_from_reference_and_adapter_selection_and_fork():
    from d3il_amd.agents import RowwiseAgent, as_batched
    agent = fake_agent()
    assert P.IBCPolicy.matches(agent) and not P.BeTPolicy.matches(agent) and not P.DDPMGPTPolicy.matches(agent)
    others = {"the corrected sampler": fake_agent(sampler=CorrectLangevinMCMCSampler()), "exponential schedule": fake_agent(sampler=LangevinMCMCSampler(poly=False)),
              "goal conditioned": fake_agent(goal=True), "derivative-free": fake_agent(sampler=DerivativeFreeOptimizer()), "vision model": fake_agent(model=EBMConvMLP()),
              "relu": fake_agent(model=EBMMLP(act="ReLU")), "norm": fake_agent(model=EBMMLP(use_norm=True)), "spectral norm": fake_agent(model=EBMMLP(spectral=True)),
              "too many iterations": fake_agent(sampler=LangevinMCMCSampler(iters=32))}
    for name, other in others.items():
        assert not P.IBCPolicy.matches(other), name
        assert isinstance(as_batched(other, 2), RowwiseAgent), name
    assert isinstance(as_batched(types.SimpleNamespace(predict=lambda s: s), 2), RowwiseAgent)
    pol = as_batched(agent, 4)
    assert isinstance(pol, P.IBCPolicy) and pol.K == K and pol.S == S and pol.A == A and pol.obs_dim == OBS and pol.steps == G["ibc_steps"].tolist()
    # the converted agent replays the golden rows
    b = Banks()
    pol = P.IBCPolicy.from_reference(agent, **b.kw())
    a = pol.predict_batch(torch.as_tensor(G["ibc_obs"][:, 0])).numpy().astype(np.float64)
    assert float(np.abs(a - G["ibc_ref64"][:, 0]).max()) <= 4 * D
    single = P.IBCPolicy.from_reference(fake_agent(sampler=LangevinMCMCSampler(second=False)))
    assert single.K == ITER and single.steps == G["ibc_steps"].tolist()[:ITER]
    # EMA: the shadow parameters are what runs
    shadow = [p.detach() * 0.5 for p in agent.model.mlp.parameters()]
    agent_ema = fake_agent(ema=True)
    agent_ema.ema_helper = types.SimpleNamespace(shadow_params=shadow)
    pe = P.IBCPolicy.from_reference(agent_ema)
    assert all(torch.equal(p, s) for p, s in zip(pe.model.parameters(), shadow))
    # fork: network shared, step word and packed buffers its own
    twin = pol.fork()
    assert twin.model is pol.model and twin._t is not pol._t and int(twin._t) == int(pol._t) == 1 and twin._packed is not pol._packed
    twin.predict_batch(torch.as_tensor(G["ibc_obs"][:, 1]))
    assert int(twin._t) == 2 and int(pol._t) == 1
    with pytest.raises((AssertionError, RuntimeError)):
        pol.predict_batch(torch.zeros(2, OBS + 1))


def test_a_rollout_range_is_a_slice_of_the_whole():
    obs = torch.as_tensor(G["ibc_obs"])
    whole, part = golden_policy("cpu", seed=5), golden_policy("cpu", seed=5)
    whole.record = part.record = True
    part.set_rollout_range(1, 2)
    for s in range(2):
        a, b = whole.predict_batch(obs[:, s]), part.predict_batch(obs[1:3, s])
        assert torch.equal(whole.last_x0[1:3], part.last_x0) and torch.equal(whole.last_noise[:, 1:3], part.last_noise) and torch.equal(whole.last_u[1:3], part.last_u)
        assert np.array_equal(whole.last_u.numpy(), P.ibc_pick_uniforms(5, 0, 4, s))
        assert np.array_equal(whole.last_noise[3].numpy(), P.ibc_normals(5, 0, 4, s, 3, A).astype(np.float32))
        assert torch.equal(whole.last_x0, whole.lo + torch.as_tensor(P.ibc_start_uniforms(5, 0, 4, s, A)) * (whole.hi - whole.lo))
        same = whole.last_picks[1:3] == part.last_picks
        assert float((a[1:3] - b)[same].abs().max()) <= 4 * D      # (torch's CPU GEMM rounds a 128-row and a 256-row batch differently; the draws are identical)
    assert bool(((whole.last_x >= whole.lo) & (whole.last_x <= whole.hi)).all())


def test_host_generators():
    """The words are Philox4x32-10 of the stated counters; every counter field changes them; moments over 2^20 draws within 5 sigma."""
    seed, off, t, k = 0x1234567890ABCDEF, (1 << 32) - 3, 7, 5
    for kind in (0, 1):
        w = P.ibc_words(seed, off, 3, t, kind, k if kind else 0)
        assert w.shape == (3, 64, 2, 4) and w.dtype == np.uint32
        for n in range(3):
            ge = off + n
            for s in (0, 1, 17, 63):
                for q in range(2):
                    want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, ge & 0xFFFFFFFF, ge >> 32, t, 0x49420000 | kind << 14 | (k if kind else 0) << 8 | s << 2 | q)
                    assert [int(x) for x in want] == w[n, s, q].tolist()
    w = P.ibc_words(seed, off, 3, t, 1, k)
    z = P.ibc_normals(seed, off, 3, t, k, 8)
    r = w[1, 3, 1].astype(np.float64)
    u1, u2 = (np.floor(r[2] / 256) + 1) / 2 ** 24, np.floor(r[3] / 256) / 2 ** 24
    assert z[1, 3, 6] == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2) and z[1, 3, 7] == np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)
    assert np.array_equal(P.ibc_normals(seed, off, 3, t, k, 3), z[:, :, :3])
    u = P.ibc_start_uniforms(seed, off, 3, t, 8)
    w0 = P.ibc_words(seed, off, 3, t, 0, 0)
    assert u.dtype == np.float32 and u[2, 9, 5] == np.float32((int(w0[2, 9, 1, 1]) >> 8) / 2.0 ** 24) and np.array_equal(P.ibc_start_uniforms(seed, off, 3, t, 2), u[:, :, :2])
    pu = P.ibc_pick_uniforms(seed, off, 3, t)
    want = P.philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, (off + 1) & 0xFFFFFFFF, (off + 1) >> 32, t, 0x49420000 | 2 << 14)
    assert pu.dtype == np.float32 and pu[1] == np.float32((int(want[0]) >> 8) / 2.0 ** 24)
    # every field of the counter matters, and no two (kind, k, s, q) of an environment share a word
    base = P.ibc_words(seed, 0, 4, t, 1, k)
    for other in (P.ibc_words(seed + 1, 0, 4, t, 1, k), P.ibc_words(seed, 4, 4, t, 1, k), P.ibc_words(seed, 0, 4, t + 1, 1, k), P.ibc_words(seed, 0, 4, t, 1, k + 1),
                  P.ibc_words(seed, 0, 4, t, 0, k), P.ibc_words(seed, 0, 4, t, 2, k), P.ibc_words(seed ^ (1 << 40), 0, 4, t, 1, k), P.ibc_words(seed, 1 << 32, 4, t, 1, k)):
        assert not np.isin(other, base).any()
    assert np.array_equal(P.ibc_words(seed, 1, 3, t, 1, k), base[1:])
    assert len({tuple(x) for x in base.reshape(-1, 4)}) == 4 * 64 * 2
    tags = {0x49420000 | kind << 14 | kk << 8 | s << 2 | q for kind in range(3) for kk in range(64) for s in range(64) for q in range(2)}
    assert 0 not in tags and P.BET_TAG not in tags and not any((tag & 0xFFFF0000) == P.DDPM_GPT_TAG for tag in tags) and len(tags) == 3 * 64 * 64 * 2
    # moments over 2^20 draws
    big = np.concatenate([P.ibc_normals(3, 0, 1024, 0, kk, 8).reshape(-1) for kk in range(2)])
    n = big.size
    assert n >= 1 << 20 and np.isfinite(big).all()
    print("moments over %d normals: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e)" % (n, big.mean(), 5 / np.sqrt(n), big.var() - 1, 5 * np.sqrt(2 / n)))
    assert abs(big.mean()) < 5 / np.sqrt(n) and abs(big.var() - 1) < 5 * np.sqrt(2 / n)
    uu = np.concatenate([P.ibc_start_uniforms(3, 0, 1024, tt, 8).reshape(-1).astype(np.float64) for tt in range(2)])
    m = uu.size
    print("moments over %d uniforms: mean - 1/2 %.3e (bar %.3e), var - 1/12 %.3e (bar %.3e)" % (m, uu.mean() - 0.5, 5 / np.sqrt(12 * m), uu.var() - 1 / 12, 5 / np.sqrt(180 * m)))
    assert m >= 1 << 20 and uu.min() >= 0.0 and uu.max() <= 1 - 2.0 ** -24
    assert abs(uu.mean() - 0.5) < 5 / np.sqrt(12 * m) and abs(uu.var() - 1 / 12) < 5 / np.sqrt(180 * m)


@pytest.mark.parametrize("hidden,blocks,obs,A_", [(128, 3, 4, 2), (256, 2, 20, 8), (128, 0, 6, 3)])
def test_packed_transposes(hidden, blocks, obs, A_):
    """wT_blk [layer][To][t][lane (g, i)][r] = W^T[16 To + i][16 t + 4 g + r] = W[16 t + 4 g + r][16 To + i]; wT_act [t][lane (g, i)][r] = W_in[16 t + 4 g + r][obs + i]."""
    pol = P.IBCPolicy.random(obs, A_, device="cpu", seed=3, hidden_dim=hidden, n_blocks=blocks)
    pk = pol._pack()
    lin_in, blks, _ = pol.model._parts()
    NT = hidden // 16
    assert pk["wT_act"].shape == (NT, 64, 4) and pk["wT_blk"].shape == (max(2 * blocks, 1), NT, NT, 64, 4) and pk["w_blk"].shape == pk["wT_blk"].shape
    rng = np.random.default_rng(0)
    for _ in range(400):
        To, t, g, i, r = (int(rng.integers(0, m)) for m in (NT, NT, 4, 16, 4))
        want = float(lin_in.weight[16 * t + 4 * g + r, obs + i]) if i < A_ else 0.0
        assert float(pk["wT_act"][t, 16 * g + i, r]) == want
        for b, (l1, l2) in enumerate(blks):
            for j, l in enumerate((l1, l2)):
                assert float(pk["wT_blk"][2 * b + j, To, t, 16 * g + i, r]) == float(l.weight.t()[16 * To + i, 16 * t + 4 * g + r]) == float(l.weight[16 * t + 4 * g + r, 16 * To + i])
                assert float(pk["w_blk"][2 * b + j, To, t, 16 * g + i, r]) == float(l.weight[16 * To + i, 16 * t + 4 * g + r])


@pytest.mark.parametrize("hidden,nb,obs,A_", [(128, 3, 4, 2), (256, 2, 20, 8)])
def test_operand_scheme_reproduces_energy_and_gradient(hidden, nb, obs, A_):
    """csrc/policy_ibc.h restated tile by tile in f64 NumPy on the packed buffers - D[i][j] = sum_k A[i][k] B[k][j] per 16 x 16 x 4 step, lane (g, i) holds A[i][g],
    lane (g, j) holds B[g][j] and D[4 g + r][j] - for one row tile: forward on w_in / w_blk / w_out, backward from the output row of w_out through wT_blk to wT_act,
    the gather of component 4 g' + r from lane (g', j), register r.  Equals ``resmlp_energy_and_grad``: the packed transposes put W^T's output tile To where the
    forward pass left pre-activation To."""
    A = A_
    torch.manual_seed(0)
    pol = P.IBCPolicy.random(obs, A, device="cpu", hidden_dim=hidden, n_blocks=nb, weight_gain=1.6)
    pk = {k: (v.double().numpy() if torch.is_tensor(v) else v) for k, v in pol._pack().items()}
    NT = hidden // 16
    rows = torch.randn(16, obs + A, dtype=torch.float64)
    m = pol.model.double()
    e_ref, g_ref = P.resmlp_energy_and_grad(m, rows, obs)
    def to_b(X):      # [16, H] -> [t][lane][r]
        out = np.zeros((NT, 64, 4))
        for t in range(NT):
            for g in range(4):
                for j in range(16):
                    out[t, 16 * g + j] = X[j, 16 * t + 4 * g: 16 * t + 4 * g + 4]
        return out
    def tile(wt, xin):      # wt [t][lane][r] (one output tile), xin [t][lane][r] -> D regs [lane][r']
        D = np.zeros((16, 16))
        for t in range(NT):
            for r in range(4):
                Amat = wt[t, :, r].reshape(4, 16)      # [k=g][i]
                Bmat = xin[t, :, r].reshape(4, 16)     # [k=g][j]
                D += Amat.T @ Bmat
        out = np.zeros((64, 4))
        for g in range(4):
            for j in range(16):
                out[16 * g + j] = D[4 * g: 4 * g + 4, j]
        return out
    def layer(wl, xin, bias=None):
        y = np.stack([tile(wl[To], xin) for To in range(NT)])      # [To][lane][r] = B-operand order of the next layer
        if bias is not None:
            for To in range(NT):
                for g in range(4):
                    y[To, 16 * g:16 * g + 16] += bias[16 * To + 4 * g: 16 * To + 4 * g + 4]
        return y
    def mish(x):
        x = torch.as_tensor(x); a, b = P._mish_and_derivative(x); return a.numpy(), b.numpy()
    # input layer: w_in [To][lane (g, i)][s] = W[16 To + i][4 s + g]; in_k[s] of lane (g, j) = row j feature 4 s + g
    R = np.zeros((16, 32)); R[:, :obs + A] = rows.numpy()
    xo = np.zeros((NT, 64, 4))
    for To in range(NT):
        D = np.zeros((16, 16))
        for s in range(7):
            Amat = pk["w_in"][To, :, s].reshape(4, 16)
            Bmat = np.stack([R[:, 4 * s + g] for g in range(4)])
            D += Amat.T @ Bmat
        for g in range(4):
            for j in range(16):
                xo[To, 16 * g + j] = D[4 * g:4 * g + 4, j] + pk["b_in"][16 * To + 4 * g:16 * To + 4 * g + 4]
    kept = []
    for b in range(nb):
        m0, d0 = mish(xo)
        u = layer(pk["w_blk"][2 * b], m0, pk["b_blk"][2 * b])
        m1, d1 = mish(u)
        xo = xo + layer(pk["w_blk"][2 * b + 1], m1, pk["b_blk"][2 * b + 1])
        kept.append((d0, d1))
    e = tile(pk["w_out"], xo)[:16, 0] + pk["b_out"][0]      # lanes (0, j), register 0
    gy = np.zeros((NT, 64, 4))
    for To in range(NT):
        for g in range(4):
            gy[To, 16 * g:16 * g + 16] = pk["w_out"][To, 16 * g]      # w_out4[To * 64 + 16 g]
    for b in reversed(range(nb)):
        d0, d1 = kept[b]
        v = layer(pk["wT_blk"][2 * b + 1], gy) * d1
        gy = gy + layer(pk["wT_blk"][2 * b], v) * d0
    acc = tile(pk["wT_act"], gy)
    ga = np.zeros((16, 8))
    for q in range(8):
        for j in range(16):
            ga[j, q] = acc[((q >> 2) << 4) + j, q & 3]
    assert float(np.abs(e - e_ref.numpy()).max()) <= 1e-12 * float(e_ref.abs().max())
    assert float(np.abs(ga[:, :A] - g_ref.numpy()).max()) <= 1e-12 * float(g_ref.abs().max()) and float(np.abs(ga[:, A:]).max() if A < 8 else 0.0) == 0.0


def test_nonfinite_state_marks_its_environment_only():
    b = Banks()
    clean, dirty = golden_policy("cpu", **b.kw()), golden_policy("cpu", **b.kw())
    obs = torch.as_tensor(G["ibc_obs"][:, 0]).clone()
    want = clean.predict_batch(obs)
    obs[2, 1] = float("nan")
    have = dirty.predict_batch(obs)
    assert dirty.last_picks.tolist()[2] == -1 and torch.isnan(have[2]).all() and torch.isfinite(have[[0, 1, 3]]).all()
    assert torch.equal(dirty.last_picks[[0, 1, 3]], clean.last_picks[[0, 1, 3]]) and float((have[[0, 1, 3]] - want[[0, 1, 3]]).abs().max()) <= 4 * D


def test_binding_has_the_headers_argument_list():
    """capi's argtypes of d3il_ibc_langevin_f32 against the declaration in include/d3il_rollout.h: count and kind (pointer / float / 64-bit / long / int) of every argument."""
    import ctypes as C
    import re
    from d3il_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "d3il_rollout.h")).read()
    decl = re.search(r"int d3il_ibc_langevin_f32\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    kind = lambda a: C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_uint64 if a.startswith("uint64_t") else C.c_long if a.startswith("long") else C.c_int
    assert len(args) == 37
    assert capi.load().d3il_ibc_langevin_f32.argtypes == [kind(a) for a in args]
