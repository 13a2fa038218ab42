"""policies.BESONativePolicy on the GPU: the golden replay of tests/test_policies_beso_native.py on cuda:0 (torch blocks + step kernel), the 120-wide policy with the
matrix-core blocks + step kernel against the f32 blocks + torch glue on the same Philox stream, the policy as one captured graph, Stacking_Sim in one and two
sub-batches - the test this policy exists for -, and the range guard's launch count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAG_BAD = (1 << 16) | (1 << 18)      # solver failure, contact overflow
S = 16
# tests/test_gpu_policies_ddpm_gpt.py derives its bar from the BeT comparison's - max |difference| below 2e-5 of the largest magnitude per forward, ten-fold for the action
# behind head and output scaling: 2e-5 * 1.5 (scaled-space range) * 0.002 (action_scale) * 10 - times the number of forwards in the chain.  This sampler runs S = 16.
BAR_PATHS = 2e-5 * 1.5 * 0.002 * 10 * S


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_golden_replay_on_the_device(dev, monkeypatch):
    """The bar of the CPU replay: every one of the 48 rows within 4 D of the reference's f64 table (D: the reference's own f32 error, stored in the fixture).  The
    fixture net is 32 wide: torch blocks + the step kernel's run-time-width instantiation.  Measured: 5.42e-09 = 1.29 D (D = 4.194e-09)."""
    from tests.test_policies_beso_native import D, replay
    monkeypatch.delenv("D3IL_POLICY_BESO_STEP", raising=False)
    w64, w32, pol = replay(dev)
    print("golden replay (cuda): D %.3e, worst |action - f64 reference| %.3e (%.2f D), worst |action - f32 reference| %.3e" % (D, w64, w64 / D, w32))
    assert pol.step_kernel_ok(dev) and pol.last_bad.tolist() == [0] * 6
    assert w64 <= 4 * D


def test_fused_blocks_and_step_kernel_against_the_f32_path(dev, monkeypatch):
    """The Stacking shape (120 wide, 6 layers, 6 heads, window 5, S = 16) at 130 environments, 8 steps (growing window, then full) with a restart of two lanes.
    Split-f16 blocks + step kernel against the same policy under D3IL_POLICY_GEMM=f32 and D3IL_POLICY_BESO_STEP=0 with the same seed: the same Philox words, the
    kernel's f32 Box-Muller against the host's f64 one rounded to f32.  Bar: BAR_PATHS (above), 9.6e-06.  Measured on one MI355X: worst |action difference| 1.69e-09, the ring
    (times action_scale) 1.67e-09, the two Box-Muller forms 1.43e-06 apart, 93 % of the action components inside the bounds."""
    from d3il_amd import policies as P
    n, steps, seed = 130, 8, 3
    g = torch.Generator().manual_seed(100 + seed)
    obs = (torch.randn(n, steps, 20, generator=g) * 0.5).to(dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev); mask[5:7] = 1
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.delenv("D3IL_POLICY_BESO_STEP", raising=False)
    fused = P.BESONativePolicy.random(20, 8, device=dev, seed=seed, policy_seed=17)
    fused.record = True
    assert fused.f16x3_blocks and fused.step_kernel_ok(dev)
    got = []
    for t in range(steps):
        if t == 3:
            fused.begin_episodes(mask)
        a = fused.predict_batch(obs[:, t]).clone()
        got.append((a, {k: v.clone() for k, v in fused.last_noise.items()}))
    assert fused.last_bad.sum().item() == 0 and fused.hist.len.tolist() == [5] * n and int(fused._t) == steps
    monkeypatch.setenv("D3IL_POLICY_GEMM", "f32")
    monkeypatch.setenv("D3IL_POLICY_BESO_STEP", "0")
    plain = P.BESONativePolicy.random(20, 8, device=dev, seed=seed, policy_seed=17)
    plain.record = True
    assert not plain.f16x3_blocks and not plain.step_kernel_ok(dev)
    worst_a = worst_n = worst_r = 0.0
    inside = []
    for t in range(steps):
        if t == 3:
            plain.begin_episodes(mask)
        a = plain.predict_batch(obs[:, t])
        worst_a = max(worst_a, float((got[t][0] - a).abs().max()))
        for d in range(S):
            worst_n = max(worst_n, float((got[t][1][d] - plain.last_noise[d]).abs().max()))
        inside.append(float(((a.abs() < 1.5 * 0.002 - 1e-9).float().mean())))
    worst_r = float((fused.a_hist - plain.a_hist).abs().max()) * 0.002
    print("fused vs f32 path: worst |action difference| %.3e (bar %.3e), worst |noise difference| %.3e, worst |ring difference| x action_scale %.3e, action components "
          "inside the bounds %.2f" % (worst_a, BAR_PATHS, worst_n, worst_r, float(np.mean(inside))))
    assert worst_n < 1e-5 and float(np.mean(inside)) > 0.05      # (not everything sits on the bounds)
    assert worst_a < BAR_PATHS and worst_r < BAR_PATHS


def test_captured_policy(dev, monkeypatch):
    """CapturedPolicy(BESONativePolicy), captured with the runtime's default hardware queues: the warm-up calls of the capture do not count as steps (step word, window
    and action ring are put back), every replay draws the next step's noise (the step word is advanced on the device inside the graph: once per step), and the actions
    are those of the uncaptured policy with the same seed and step sequence - the same kernels on the same inputs, bit for bit."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.delenv("D3IL_POLICY_BESO_STEP", raising=False)
    monkeypatch.delenv("D3IL_POLICY_RANGE_GUARD", raising=False)
    n, steps = 64, 7
    obs = (torch.randn(n, steps, 20, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    eager = P.BESONativePolicy.random(20, 8, device=dev, seed=4, policy_seed=11)
    inner = P.BESONativePolicy.random(20, 8, device=dev, seed=4, policy_seed=11)
    eager.record = inner.record = True
    cap = P.CapturedPolicy(inner)
    seen = []
    for t in range(steps):
        if t == 3:                      # lanes 5 and 6 start a new episode: both policies restart their windows
            m = torch.zeros(n, dtype=torch.uint8, device=dev); m[5:7] = 1
            cap.begin_episodes(m); eager.begin_episodes(m)
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t]).clone()
        torch.cuda.synchronize()
        assert int(inner._t) == t + 1 == int(eager._t), t                     # once per step, whatever the capture did before
        z = inner.last_noise[0][:, 0].cpu().numpy().copy()
        assert float(np.abs(z - P.beso_normals(11, 0, n, t, 0, 5, 8)[:, 0]).max()) < 1e-5, t      # step t's init draw
        assert all(not np.array_equal(z, s) for s in seen)
        seen.append(z)
        for d in range(S):
            assert torch.equal(inner.last_noise[d], eager.last_noise[d]), (t, d)
        dd = float((have - want).abs().max())
        assert dd == 0.0, (t, dd)
        assert torch.equal(inner.a_hist, eager.a_hist), t
    assert cap._g is not None and inner.hist.len.tolist() == [5] * 5 + [4, 4] + [5] * (n - 7)      # (the restarted lanes have seen steps 3 .. 6)
    assert inner.last_bad.sum().item() == 0
    twin = cap.fork()
    assert twin.inner.model is inner.model and twin.inner.hist is None and twin.inner.a_hist is None and twin._g is None
    # the torch glue draws on the host: it refuses to be captured
    monkeypatch.setenv("D3IL_POLICY_BESO_STEP", "0")
    with pytest.raises(RuntimeError, match="cannot be captured"):
        P.CapturedPolicy(P.BESONativePolicy.random(20, 8, device=dev, seed=4, policy_seed=11)).predict_batch(obs[:, 0])


def test_range_guard_counts_the_launches_of_the_blocks(dev, monkeypatch):
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.delenv("D3IL_POLICY_RANGE_GUARD", raising=False)
    pol = P.BESONativePolicy.random(20, 8, device=dev, seed=4)
    obs = (torch.randn(64, 20, generator=torch.Generator().manual_seed(9)) * 0.5).to(dev)
    pol.predict_batch(obs)
    with P.RangeGuard(dev) as guard:
        pol.predict_batch(obs)
        rep = pol.range_report()
    assert rep["launches"] == S * 6 * 2 and rep["clipped"] == 0 and rep["nonfinite"] == 0 and rep["weights_out_of_range"] == 0, rep      # S steps x 6 blocks x (attention half + MLP half)
    assert guard.read()["launches"] == S * 6 * 2


def _recording_policy(P, dev, log):
    """A random-weight BESONativePolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, init noise, actions)."""
    class Rec(P.BESONativePolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, torch.stack([self.last_noise[d] for d in range(S)], dim=1).cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.BESONativePolicy.random(20, 8, device=dev, seed=6, policy_seed=21)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    pol.record = True
    return pol


def _by_step(log, n):
    out = {}
    for t, off, z, a in log:
        Z, Aa = out.setdefault(t, (np.zeros((n,) + z.shape[1:], np.float32), np.zeros((n, a.shape[1]), np.float32)))
        Z[off:off + len(z)], Aa[off:off + len(z)] = z, a
    return out


@pytest.mark.parametrize("n", [64, 128])
def test_stacking_sim_gives_the_same_actions_and_tables_in_one_and_two_sub_batches(dev, n, monkeypatch):
    """Stacking_Sim (obs 20 -> 8) with a random-weight BESONativePolicy, episodes capped at 12 steps (the DDPM-GPT test's length), n_sub_batches 1 and 2: the noise is
    keyed by the global environment index (set_rollout_range -> env_offset), every kernel of the chain works row by row, so the two runs give the same noise and the
    same actions BIT FOR BIT for every rollout and step, and the same (success, mode) tables - what BESOPolicy on the device generator cannot give.  A sub-batch holds
    at least one wavefront of environments (envs/sub_batch.plan): at 64 environments n_sub_batches = 2 still runs as ONE batch, at 128 the batch is really cut in two."""
    from d3il_amd import policies as P
    from d3il_amd.simulation.stacking_sim import Stacking_Sim
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.delenv("D3IL_POLICY_BESO_STEP", raising=False)
    steps = 12
    res = {}
    for nsub in (1, 2):
        log = []
        sim = Stacking_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_contexts=8, n_trajectories_per_context=n // 8, max_steps_per_episode=steps, n_sub_batches=nsub)
        sim.test_agent(_recording_policy(P, dev, log))
        r = sim.last_rollout
        tables = (r["counts"].copy(), r["mode"].cpu().numpy(), r["success"].cpu().numpy())
        assert not bool((r["flags"] & FLAG_BAD).any())
        assert len({off for _, off, *_ in log}) == (nsub if n >= 128 else 1) and r["mode"].shape[0] == n
        res[nsub] = (tables, _by_step(log, n))
    for x, y in zip(res[1][0], res[2][0]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    one, two = res[1][1], res[2][1]
    assert sorted(one) == sorted(two) and len(one) >= steps
    for t in sorted(one):
        assert np.array_equal(one[t][0].view(np.uint32), two[t][0].view(np.uint32)), t          # the same noise for every rollout, however the batch is cut
        assert np.array_equal(one[t][1].view(np.uint32), two[t][1].view(np.uint32)), t          # and the same actions, bit for bit
    assert len(np.unique(np.concatenate([one[t][1] for t in one]))) > 20                     # not one action all along
