"""policies.BeTMLPPolicy on the GPU: the golden replay of tests/test_policies_bet_mlp.py on cuda:0 through the kernel, the kernel against torch's layers
(D3IL_POLICY_BET_MLP_FUSED=0) on the same Philox stream, CapturedPolicy around it, and Avoiding_Sim / Sorting_Sim in one and in two sub-batches."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAG_BAD = (1 << 16) | (1 << 18)      # solver failure, contact overflow


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_golden_replay_through_the_kernel(dev, monkeypatch):
    from tests.test_policies_bet_mlp import D, replay
    monkeypatch.delenv("D3IL_POLICY_BET_MLP_FUSED", raising=False)
    worst, pol = replay(dev)      # (asserts the golden bin on every row)
    print("golden replay (kernel): actions %.3e = %.2f D (D %.3e)" % (worst, worst / D, D))
    assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None      # the kernel ran, not torch's layers
    assert worst <= 4 * D
    assert int(pol._t) == 4


def test_kernel_equals_torchs_layers_on_the_same_philox_stream(dev, monkeypatch):
    """130 environments x 4 steps, hidden 256 / 4 blocks, obs 20 -> 8: both paths take the same uniform (24 bits, exact in f32).  EVERY row is compared: its
    probabilities against the f64 softmax, its action against the f64 restatement evaluated at the bin the row drew, and its bin against the f64 rule - equal, except
    that a row whose u sits within BET_MLP_EDGE of an edge of its f64 CDF (520 rows x 64 edges x 2 EDGE: about seven of them) may fall to either side of that edge
    in an f32 arithmetic and must draw one of the two bins next to it.  Bar: 4 x the deviation of torch's f32 layers from f64, measured the same way."""
    from d3il_amd import policies as P
    n, T = 130, 4
    obs = (torch.randn(n, T, 20, generator=torch.Generator().manual_seed(8)) * 0.7).to(dev)
    mk = lambda: P.BeTMLPPolicy.random(20, 8, device=dev, seed=4, hidden_dim=256, n_blocks=4, policy_seed=13)
    fused, plain = mk(), mk()
    fused.record = plain.record = True
    ref = copy.copy(plain)
    ref.model = copy.deepcopy(plain.model).double()
    d = lambda v: v.double()
    ar = torch.arange(n, device=dev)

    def actions64(out64, bins):      # steps 6 and 7 in f64 at given bins
        v = d(ref.centers)[bins.long()] + out64[:, 64:].reshape(n, 64, 8)[ar, bins.long()]
        return torch.minimum(torch.maximum(v, d(ref.lo)), d(ref.hi)) * d(ref.out_scale) + d(ref.out_shift)

    worst = yard = worst_lp = yard_lp = 0.0
    near_rows = split_rows = 0
    for t in range(T):
        monkeypatch.delenv("D3IL_POLICY_BET_MLP_FUSED", raising=False)
        a = fused.predict_batch(obs[:, t])
        assert fused._packed.key is not None
        monkeypatch.setenv("D3IL_POLICY_BET_MLP_FUSED", "0")
        b = plain.predict_batch(obs[:, t])
        assert plain._packed.key is None
        u_host = torch.as_tensor(P.bet_mlp_uniforms(13, 0, n, t)).to(dev)
        assert torch.equal(plain.last_u, u_host) and torch.equal(fused.last_u, u_host)      # bit for bit
        out64 = d(ref.scaler.scale_input(obs[:, t]))
        for layer in ref.model.layers:
            out64 = layer(out64)
        p64 = torch.softmax(out64[:, :64], dim=1)
        cdf = torch.cumsum(p64, dim=1)
        bins64 = (cdf <= d(u_host).unsqueeze(1)).sum(dim=1).clamp_max(63).to(torch.int32)
        near = (cdf - d(u_host).unsqueeze(1)).abs().min(dim=1).values < P.BET_MLP_EDGE
        near_rows += int(near.sum())
        for pol in (fused, plain):
            assert (pol.last_bins >= 0).all() and torch.equal(pol.last_bins[~near], bins64[~near])
            assert bool(((pol.last_bins[near] - bins64[near]).abs() <= 1).all())
        split_rows += int((fused.last_bins != plain.last_bins).sum())
        yard = max(yard, float((d(b) - actions64(out64, plain.last_bins)).abs().max()))
        worst = max(worst, float((d(a) - actions64(out64, fused.last_bins)).abs().max()))
        yard_lp = max(yard_lp, float((d(plain.last_probs).log() - p64.log()).abs().max()))
        worst_lp = max(worst_lp, float((d(fused.last_probs).log() - p64.log()).abs().max()))
    print("kernel against f64: actions %.3e, torch f32 %.3e -> %.2f yardsticks; log-probabilities %.3e, torch f32 %.3e -> %.2f yardsticks; rows within EDGE of a CDF edge: %d of %d, "
          "rows on which the two f32 paths drew different bins: %d" % (worst, yard, worst / yard, worst_lp, yard_lp, worst_lp / yard_lp, near_rows, n * T, split_rows))
    assert yard > 0 and worst <= 4 * yard
    assert yard_lp > 0 and worst_lp <= 4 * yard_lp
    assert int(fused._t) == T == int(plain._t)


def test_captured_policy_replays_the_kernel_with_fresh_draws(dev, monkeypatch):
    """CapturedPolicy(BeTMLPPolicy) with the runtime's default hardware queues: replay = eager bit for bit over 5 steps, a fresh draw per replay, the step word
    advances once per step (warm-up and capture do not count); the torch path refuses the capture."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_BET_MLP_FUSED", raising=False)
    n, T = 64, 5
    obs = (torch.randn(n, T, 4, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.BeTMLPPolicy.random(4, 2, device=dev, seed=5, hidden_dim=128, n_blocks=3, policy_seed=17)
    eager, inner = mk(), mk()
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    seen = []
    for t in range(T):
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        assert torch.equal(have, want), t
        assert torch.equal(inner.last_bins, eager.last_bins) and torch.equal(inner.last_u, eager.last_u), t
        assert np.array_equal(inner.last_u.cpu().numpy(), P.bet_mlp_uniforms(17, 0, n, t)), t
        u = inner.last_u.cpu().numpy().copy()
        assert all(not np.array_equal(u, s) for s in seen)
        seen.append(u)
        assert int(inner._t) == t + 1 == int(eager._t)
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    twin = cap.fork()
    assert twin.inner.model is inner.model and twin._g is None
    # torch's layers take their Philox numbers from the host: that path refuses the capture
    monkeypatch.setenv("D3IL_POLICY_BET_MLP_FUSED", "0")
    with pytest.raises(RuntimeError):
        mk().captured().predict_batch(obs[:, 0])


def _recording_policy(P, dev, obs_dim, A, log):
    """A random-weight BeTMLPPolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, u, bins, actions)."""
    class Rec(P.BeTMLPPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.last_u.cpu().numpy().copy(), self.last_bins.cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.BeTMLPPolicy.random(obs_dim, A, device=dev, seed=6, hidden_dim=128, n_blocks=3, policy_seed=21)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, u, b, a in log:
        U, B, Aa = out.setdefault(t, (np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, a.shape[1]), np.float32)))
        U[off:off + len(u)], B[off:off + len(u)], Aa[off:off + len(u)] = u, b, a
    return out


@pytest.mark.parametrize("task", ["avoiding", "sorting"])
def test_sims_give_the_same_actions_and_tables_in_one_and_two_sub_batches(dev, task, monkeypatch):
    """Avoiding_Sim (obs 4 -> 2) and Sorting_Sim (obs 16 -> 2) with a random-weight BeTMLPPolicy, 128 environments, episodes capped at 12 steps, n_sub_batches 1 and
    2: every draw is keyed by the global environment index (set_rollout_range -> env_offset) and rows do not depend on the launch, so the two runs give the same
    uniforms, bins and actions bit for bit and the same (success, mode) tables."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_BET_MLP_FUSED", raising=False)
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
        assert np.array_equal(one[t][0], P.bet_mlp_uniforms(21, 0, n, t)), t
        assert np.array_equal(one[t][0].view(np.uint32), two[t][0].view(np.uint32)) and np.array_equal(one[t][1], two[t][1]), t
        assert np.array_equal(one[t][2].view(np.uint32), two[t][2].view(np.uint32)), t
        assert (one[t][1] >= 0).all() and (one[t][1] < 64).all()
    assert np.isfinite(np.concatenate([one[t][2] for t in one])).all()
    assert len(np.unique(np.concatenate([one[t][1] for t in one]))) > 10
