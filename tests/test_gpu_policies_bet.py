"""policies.BeTPolicy on the GPU: the golden replay of tests/test_policies_bet.py on cuda:0 (torch trunk + head kernel), the 120-wide policy with the matrix-core
trunk + head kernel against the f32 trunk + torch tail, the policy as one captured graph, and Stacking_Sim / Sorting_Sim in one and two sub-batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAG_BAD = (1 << 16) | (1 << 18)      # solver failure, contact overflow


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class Table:
    """uniform_fn replaying column t of a [n, T] table at call t."""

    def __init__(self, table):
        self.table, self.call = table, 0

    def __call__(self, n):
        self.call += 1
        return self.table[:n, self.call - 1]


def test_golden_replay_on_the_device(dev):
    """Same bars as on the CPU (tests/test_policies_bet.py): bins identical on every row, actions and last-token logits (here: log-probabilities, what the head kernel
    returns) within 5e-6 of the reference's.  The fixture net is 32 wide: torch trunk + fused head."""
    from tests.test_policies_bet import BAR, replay
    same, worst_a, worst_l, pol = replay(dev)
    print("golden replay (cuda): worst |action - reference| %.3e, worst |log p - reference| %.3e" % (worst_a, worst_l))
    assert pol.last_logits is None and pol.last_probs is not None and pol.last_probs.is_cuda      # the head kernel ran
    assert same and worst_a < BAR and worst_l < BAR


def test_fused_trunk_and_head_against_the_f32_path(dev, monkeypatch):
    """The Stacking / Sorting-4 shape (120 wide, 6 layers, 6 heads) at 130 environments (three workgroups of the attention kernel, the last ragged; 130 rows = five
    workgroups of the head kernel, the fifth with two rows), window 5, 8 steps (growing window, then full).  Split-f16 trunk + head kernel against the same policy under
    D3IL_POLICY_GEMM=f32 and D3IL_POLICY_BET_HEAD=0 with the same u.  Logits (as log-probabilities) by the rule of tests/test_policies_f16x3.py
    test_block_in_both_gemm_modes_and_against_torch: max |difference| / max |logit| < 2e-5.  Bins equal on every row whose u is farther from an edge of the f32 path's
    normalised CDF than 10 x the measured deviation; at most 2 % of the rows may be left out (seed 3: 5 of 1040 rows lie within 1e-4 of an edge, 14 within 2e-4, computed
    with the CPU tail)."""
    from d3il_amd import policies as P
    n, T, seed = 130, 8, 3
    g = torch.Generator().manual_seed(100 + seed)
    obs = (torch.randn(n, T, 20, generator=g) * 0.5).to(dev)
    u = torch.randint(0, 1 << 24, (n, T), generator=g).float() / float(1 << 24)
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.delenv("D3IL_POLICY_BET_HEAD", raising=False)
    fused = P.BeTPolicy.random(20, 8, device=dev, seed=seed, uniform_fn=Table(u))
    fused.record = True
    assert fused.f16x3_blocks
    got = []
    for t in range(T):
        a = fused.predict_batch(obs[:, t]).clone()
        assert fused.last_logits is None      # the head kernel
        got.append((a, fused.last_bins.clone(), fused.last_probs.clone()))
    monkeypatch.setenv("D3IL_POLICY_GEMM", "f32")
    monkeypatch.setenv("D3IL_POLICY_BET_HEAD", "0")
    plain = P.BeTPolicy.random(20, 8, device=dev, seed=seed, uniform_fn=Table(u))
    plain.record = True
    assert not plain.f16x3_blocks
    dev_logit, scale, left_out, worst_a = 0.0, 0.0, 0, 0.0
    per_step = []
    for t in range(T):
        a = plain.predict_batch(obs[:, t])
        assert plain.last_logits is not None
        logp = torch.log_softmax(plain.last_logits.double(), dim=1)
        d = float((got[t][2].double().log() - logp).abs().max())
        per_step.append((d, a.clone(), plain.last_bins.clone(), torch.cumsum(plain.last_probs.double(), dim=1)))
        dev_logit, scale = max(dev_logit, d), max(scale, float(plain.last_logits.abs().max()))
    for t in range(T):
        d, a, bins, cdf = per_step[t]
        far = (cdf - u[:, t:t + 1].to(dev).double()).abs().min(dim=1).values > 10 * dev_logit
        left_out += int((~far).sum())
        assert torch.equal(got[t][1][far], bins[far]), t
        same = far & (got[t][1] == bins)
        worst_a = max(worst_a, float((got[t][0][same] - a[same]).abs().max()))
    print("logit deviation fused vs f32 path: %.3e (max |logit| %.2f, ratio %.2e); rows left out of the bin comparison: %d of %d; worst |action difference| %.3e" % (
        dev_logit, scale, dev_logit / scale, left_out, n * T, worst_a))
    assert dev_logit / scale < 2e-5
    assert left_out <= 0.02 * n * T
    assert worst_a < 2e-5 * 1.5 * 0.002 * 10      # scaled-space range 1.5, action_scale 0.002: the same relative rule, ten-fold (centre + offset, then the output scaling)


def test_captured_policy(dev, monkeypatch):
    """CapturedPolicy(BeTPolicy): the warm-up calls of the capture do not count as steps, every replay draws the next step's u (the step word is advanced on the device
    inside the graph), the actions are those of the uncaptured policy with the same seed and step sequence, and the graph is captured again when the range guard is switched."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.delenv("D3IL_POLICY_BET_HEAD", raising=False)
    monkeypatch.delenv("D3IL_POLICY_RANGE_GUARD", raising=False)
    n, T = 64, 9
    obs = (torch.randn(n, T, 20, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    eager = P.BeTPolicy.random(20, 8, device=dev, seed=4, policy_seed=11)
    eager.record = True
    inner = P.BeTPolicy.random(20, 8, device=dev, seed=4, policy_seed=11)
    cap = P.CapturedPolicy(inner)
    seen, left_out = [], 0
    guard = P.RangeGuard(dev)
    try:
        for t in range(T):
            if t == 5:
                g_before = cap._g
                guard.reset()
                guard.enable()
            if t == 7:
                g_guarded = cap._g
                guard.disable()
            if t == 3:                      # lanes 5 and 6 start a new episode: both policies restart their windows
                m = torch.zeros(n, dtype=torch.uint8, device=dev); m[5:7] = 1
                cap.begin_episodes(m); eager.begin_episodes(m)
            want = eager.predict_batch(obs[:, t])
            have = cap.predict_batch(obs[:, t])
            torch.cuda.synchronize()
            u = inner.last_u.cpu().numpy().copy()
            assert np.array_equal(u, P.bet_uniforms(11, 0, n, t)), t          # step t, whatever the capture did before
            assert np.array_equal(u, eager.last_u.cpu().numpy())
            assert all(not np.array_equal(u, s) for s in seen)
            seen.append(u)
            cdf = torch.cumsum(eager.last_probs.double(), dim=1)
            far = (cdf - eager.last_u.unsqueeze(1).double()).abs().min(dim=1).values > 1e-4
            left_out += int((~far).sum())
            assert torch.equal(inner.last_bins[far], eager.last_bins[far]), t
            same = far & (inner.last_bins == eager.last_bins)
            assert float((have[same] - want[same]).abs().max()) < 2e-5 * 1.5 * 0.002 * 10, t
            if t == 5:
                assert cap._g is not g_before and guard.read()["launches"] > 0       # captured again, with the guarded kernels
                g_on = cap._g
            if t == 6:
                assert cap._g is g_on                                                 # nothing changed: a replay
            if t == 7:
                assert cap._g is not g_guarded                                        # guard off: captured again
    finally:
        guard.disable()
    assert inner.hist.len.tolist() == [5] * n and int(inner._t) == T == int(eager._t)
    print("captured vs eager: rows left out of the bin comparison (u within 1e-4 of an edge): %d of %d" % (left_out, n * T))
    assert left_out <= 0.02 * n * T
    twin = cap.fork()
    assert twin.inner.trunk is inner.trunk and twin.inner.hist is None and twin._g is None


def _recording_policy(P, dev, obs_dim, A, log):
    """A random-weight BeTPolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, u, bins, actions)."""
    class Rec(P.BeTPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.last_u.cpu().numpy().copy(), self.last_bins.cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.BeTPolicy.random(obs_dim, A, device=dev, seed=6, policy_seed=21)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, u, b, a in log:
        U, B, Aa = out.setdefault(t, (np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros((n, a.shape[1]))))
        U[off:off + len(u)], B[off:off + len(u)], Aa[off:off + len(u)] = u, b, a
    return out


@pytest.mark.parametrize("task", ["stacking", "sorting"])
def test_sims_give_the_same_tables_in_one_and_two_sub_batches(dev, task, monkeypatch):
    """Stacking_Sim (obs 20 -> 8) and Sorting_Sim (obs 16 -> 2) with a random-weight BeTPolicy, episodes capped at 20 steps, n_sub_batches 1 and 2: the draw is keyed by
    the global environment index (set_rollout_range -> env_offset), so the two runs draw the same u for every rollout and step and return the same tables (the property
    tests/test_subbatch_sims.py asserts for the other policies).  128 environments: a sub-batch is at least one wavefront of environments (envs/sub_batch.plan), so 64
    would run as ONE batch for n_sub_batches = 2 and compare a run with itself."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.delenv("D3IL_POLICY_BET_HEAD", raising=False)
    n, steps = 128, 20
    res = {}
    for S in (1, 2):
        log = []
        if task == "stacking":
            from d3il_amd.simulation.stacking_sim import Stacking_Sim
            sim = Stacking_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_contexts=8, n_trajectories_per_context=16, max_steps_per_episode=steps, n_sub_batches=S)
            sim.test_agent(_recording_policy(P, dev, 20, 8, log))
            r = sim.last_rollout
            tables = (r["counts"].copy(), r["mode"].cpu().numpy(), r["success"].cpu().numpy())
        else:
            from d3il_amd.simulation.sorting_sim import Sorting_Sim
            sim = Sorting_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_contexts=8, n_trajectories_per_context=16, max_steps_per_episode=steps, n_sub_batches=S)
            sim.test_agent(_recording_policy(P, dev, 16, 2, log))
            r = sim.last_rollout
            tables = (r["counts"].copy(), r["mode"].cpu().numpy(), r["success"].cpu().numpy(), r["mode_hist"].copy())
        assert not bool((r["flags"] & FLAG_BAD).any()), task
        assert len({off for _, off, *_ in log}) == S and r["mode"].shape[0] == n
        res[S] = (tables, _by_step(log, n))
    for x, y in zip(res[1][0], res[2][0]):
        assert np.array_equal(np.asarray(x), np.asarray(y)), task
    one, two = res[1][1], res[2][1]
    assert sorted(one) == sorted(two) and len(one) >= steps
    flips = 0
    for t in sorted(one):
        assert np.array_equal(one[t][0], two[t][0]), t                                  # the same u for every rollout, however the batch is cut
        assert np.array_equal(one[t][0], P.bet_uniforms(21, 0, n, t))
        flips += int((one[t][1] != two[t][1]).sum())
    print("%s: bins that differ between one and two sub-batches: %d of %d" % (task, flips, n * len(one)))
    assert flips == 0
    assert len(np.unique(np.concatenate([one[t][1] for t in one]))) > 20                # not one bin all along
