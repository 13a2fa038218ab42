"""policies.IBCPolicy on the GPU: the golden replay of tests/test_policies_ibc.py on cuda:0 through the chain kernel, the kernel against the torch-op chain
(D3IL_POLICY_IBC_FUSED=0) on the same Philox stream, CapturedPolicy around it, and Avoiding_Sim / Sorting_Sim in one and in two sub-batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAG_BAD = (1 << 16) | (1 << 18)      # solver failure, contact overflow
EDGE = 1e-4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_golden_replay_through_the_kernel(dev, monkeypatch):
    from tests.test_policies_ibc import D, DX, DE, replay
    monkeypatch.delenv("D3IL_POLICY_IBC_FUSED", raising=False)
    wa, wx, we, same, pol = replay(dev)
    print("golden replay (kernel): actions %.3e = %.2f D, final samples %.3e = %.2f D_x, energies %.3e = %.2f D_E" % (wa, wa / D, wx, wx / DX, we, we / DE))
    assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None      # the kernel ran, not the torch chain
    assert same
    assert wa <= 4 * D and wx <= 4 * DX and we <= 4 * DE
    assert int(pol._t) == 4


def test_kernel_equals_the_torch_chain_on_the_same_philox_stream(dev, monkeypatch):
    """130 environments x 4 steps, hidden 256 / 4 blocks, obs 20 -> 8: both paths draw the same start points, normals and uniforms; picks equal on every row whose u
    is farther than EDGE from an edge of the torch path's CDF (expected share left out: 63 edges x 2 x 1e-4 = 1.3 %, at most 5 %)."""
    from d3il_amd import policies as P
    n, T = 130, 4
    obs = (torch.randn(n, T, 20, generator=torch.Generator().manual_seed(8)) * 0.7).to(dev)
    mk = lambda: P.IBCPolicy.random(20, 8, device=dev, seed=4, hidden_dim=256, n_blocks=4, policy_seed=13, weight_gain=1.6)
    fused, plain = mk(), mk()
    fused.record = plain.record = True
    left_out, worst = 0, 0.0
    for t in range(T):
        monkeypatch.delenv("D3IL_POLICY_IBC_FUSED", raising=False)
        a = fused.predict_batch(obs[:, t])
        assert fused.last_x is not None and fused._packed.key is not None
        monkeypatch.setenv("D3IL_POLICY_IBC_FUSED", "0")
        b = plain.predict_batch(obs[:, t])
        assert torch.equal(fused.last_u, plain.last_u) and np.array_equal(fused.last_u.cpu().numpy(), P.ibc_pick_uniforms(13, 0, n, t))
        assert torch.equal(fused.last_x0, plain.last_x0)
        assert float((fused.last_noise - plain.last_noise).abs().max()) < 1e-5      # the kernel's f32 Box-Muller against the host's f64 one
        e = plain.last_energies.double()
        cdf = torch.cumsum(torch.softmax(-e, dim=1), dim=1)
        far = (cdf - plain.last_u.double().unsqueeze(1)).abs().min(dim=1).values > EDGE
        left_out += int((~far).sum())
        assert torch.equal(fused.last_picks[far], plain.last_picks[far]), t
        same = far & (fused.last_picks == plain.last_picks)
        worst = max(worst, float((a[same] - b[same]).abs().max() / 0.002), float((fused.last_x - plain.last_x).abs().max()))
    print("kernel vs torch chain: rows left out (u within 1e-4 of an edge) %d of %d = %.2f %%; worst |x - x| %.3e" % (left_out, n * T, 100.0 * left_out / (n * T), worst))
    assert left_out <= 0.05 * n * T
    assert int(fused._t) == T == int(plain._t)


def test_captured_policy_replays_the_kernel_with_fresh_draws(dev, monkeypatch):
    """CapturedPolicy(IBCPolicy) with the runtime's default hardware queues: replay = eager bit for bit, fresh draws per replay, the step word advances once per step
    (warm-up and capture do not count)."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_IBC_FUSED", raising=False)
    n, T = 64, 5
    obs = (torch.randn(n, T, 4, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.IBCPolicy.random(4, 2, device=dev, seed=5, hidden_dim=128, n_blocks=3, policy_seed=17)
    eager, inner = mk(), mk()
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    seen = []
    for t in range(T):
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        assert torch.equal(have, want), t
        assert torch.equal(inner.last_u, eager.last_u) and np.array_equal(inner.last_u.cpu().numpy(), P.ibc_pick_uniforms(17, 0, n, t)), t
        assert torch.equal(inner.last_picks, eager.last_picks)
        u = inner.last_u.cpu().numpy().copy()
        assert all(not np.array_equal(u, s) for s in seen)
        seen.append(u)
        assert int(inner._t) == t + 1 == int(eager._t)
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    twin = cap.fork()
    assert twin.inner.model is inner.model and twin._g is None
    # the torch chain draws on the host: it refuses the capture
    monkeypatch.setenv("D3IL_POLICY_IBC_FUSED", "0")
    with pytest.raises(RuntimeError):
        mk().captured().predict_batch(obs[:, 0])


def _recording_policy(P, dev, obs_dim, A, log):
    """A random-weight IBCPolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, u, picks, actions)."""
    class Rec(P.IBCPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.last_u.cpu().numpy().copy(), self.last_picks.cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.IBCPolicy.random(obs_dim, A, device=dev, seed=6, hidden_dim=128, n_blocks=3, policy_seed=21)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, u, b, a in log:
        U, B, Aa = out.setdefault(t, (np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros((n, a.shape[1]), np.float32)))
        U[off:off + len(u)], B[off:off + len(u)], Aa[off:off + len(u)] = u, b, a
    return out


@pytest.mark.parametrize("task", ["avoiding", "sorting"])
def test_sims_give_the_same_actions_and_tables_in_one_and_two_sub_batches(dev, task, monkeypatch):
    """Avoiding_Sim (obs 4 -> 2) and Sorting_Sim (obs 16 -> 2) with a random-weight IBCPolicy, 128 environments, episodes capped at 12 steps, n_sub_batches 1 and 2:
    every draw is keyed by the global environment index (set_rollout_range -> env_offset) and rows do not depend on the launch, so the two runs give the same
    actions bit for bit and the same (success, mode) tables."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_IBC_FUSED", raising=False)
    n, steps = 128, 12
    res = {}
    for nsub in (1, 2):
        log = []
        if task == "avoiding":
            from d3il_amd.simulation.avoiding_sim import Avoiding_Sim
            sim = Avoiding_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_trajectories=n, max_steps_per_episode=steps, n_sub_batches=nsub)
            sim.test_agent(_recording_policy(P, dev, 4, 2, log))
        else:
            from d3il_amd.simulation.sorting_sim import Sorting_Sim
            sim = Sorting_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_contexts=8, n_trajectories_per_context=16, max_steps_per_episode=steps, n_sub_batches=nsub)
            sim.test_agent(_recording_policy(P, dev, 16, 2, log))
        r = sim.last_rollout
        if task == "avoiding":
            tables = (np.asarray(r["counts"]).copy(), r["mode_code"].cpu().numpy(), r["success"].cpu().numpy(), r["n_pos"].cpu().numpy())
            assert bool(torch.isfinite(r["c_pos"]).all())
        else:
            tables = (np.asarray(r["counts"]).copy(), r["mode"].cpu().numpy(), r["success"].cpu().numpy())
            assert not bool((r["flags"] & FLAG_BAD).any())
        assert len({off for _, off, *_ in log}) == nsub and r["success"].shape[0] == n
        res[nsub] = (tables, _by_step(log, n))
    for x, y in zip(res[1][0], res[2][0]):
        assert np.array_equal(x, y), task
    one, two = res[1][1], res[2][1]
    assert sorted(one) == sorted(two) and len(one) >= steps
    for t in sorted(one):
        assert np.array_equal(one[t][0], P.ibc_pick_uniforms(21, 0, n, t)) and np.array_equal(one[t][0], two[t][0]), t
        assert np.array_equal(one[t][1], two[t][1]) and np.array_equal(one[t][2].view(np.uint32), two[t][2].view(np.uint32)), t
    assert len(np.unique(np.concatenate([one[t][1] for t in one]))) > 20
