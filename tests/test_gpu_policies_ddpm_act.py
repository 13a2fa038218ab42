"""policies.DDPMACTPolicy on the GPU: the golden replay of tests/test_policies_ddpm_act.py on cuda:0 through the chain kernel, the kernel against the torch path
(D3IL_POLICY_DDPM_ACT_FUSED=0) on the same Philox stream, CapturedPolicy around it, the NaN lane in an Avoiding step, and Avoiding_Sim / Sorting_Sim in one and in
two sub-batches."""
import copy
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SOLVER_FAIL = 1 << 16
FLAG_BAD = (1 << 16) | (1 << 18)      # solver failure, contact overflow


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", ["a", "b"])
def test_golden_replay_through_the_kernel(dev, case, monkeypatch):
    from tests.test_policies_ddpm_act import cfg, replay
    monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
    c = cfg(case)
    wa, wc, same, exact, n_edge, pol = replay(case, dev)
    print("golden replay %s (kernel): actions %.3e = %.2f D, chunks %.3e = %.2f D (D %.3e); %d chunk entries on a clamp bound" % (case, wa, wa / c.D, wc, wc / c.D, c.D, n_edge))
    assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None      # the kernel ran, not the torch path
    assert same and exact and n_edge > 0
    assert wa <= 4 * c.D and wc <= 4 * c.D
    assert int(pol._t) == c.n_steps


def test_kernel_equals_the_torch_path_on_the_same_philox_stream(dev, monkeypatch):
    """130 environments x 9 steps of the shipped shape, a begin_episodes mask at step 2: both paths keep the same counters and window lengths and draw
    from the same Philox words (the device's f32 Box-Muller against the host's f64 one rounded to f32: within 4 deviations of a torch f32 Box-Muller, 1e-5 for
    short; the same entries drawn and not drawn); no row is left out.  Yardstick of the actions: the deviation of the torch path (f32) from the same path on a double
    network fed the same f32 normals, taken here; bar 4 of them."""
    from d3il_amd import policies as P
    n, steps, T = 130, 9, 16
    obs = (torch.randn(n, steps, 10, generator=torch.Generator().manual_seed(8)) * 0.7).to(dev)
    mk = lambda **kw: P.DDPMACTPolicy.random(10, 2, device=dev, seed=4, policy_seed=13, n_envs=n, n_timesteps=T, bound=2.5, **kw)
    fused, plain = mk(), mk()
    fused.record = plain.record = True
    exact = mk()      # the f64 table: the torch path's bookkeeping on a double network, fed what the torch path draws
    exact.model = copy.deepcopy(exact.model).double()
    mask = (torch.arange(n, device=dev) % 3 == 1)
    worst = yard = wn = 0.0
    for t in range(steps):
        if t == 2:
            for p in (fused, plain, exact):
                p.begin_episodes(mask)
        monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
        a = fused.predict_batch(obs[:, t])
        assert fused._packed.key is not None
        monkeypatch.setenv("D3IL_POLICY_DDPM_ACT_FUSED", "0")
        b = plain.predict_batch(obs[:, t])
        # the same step in f64: windows, counters and grouping are the policy's own; the chain runs on the double network
        s = exact.scaler.scale_input(obs[:, t].to(torch.float32))
        exact.hist.append_(s)
        win, ln = exact.hist.padded()
        due = exact.counter >= exact.Ta
        if bool(due.any()):
            z = torch.as_tensor(np.stack([np.zeros((n, 4, 2))] + [P.ddpm_act_normals(13, 0, n, t, k, 4, 2) for k in range(1, T + 1)], axis=1), dtype=torch.float32).to(dev)
            if not hasattr(exact, "chunk64"):
                exact.chunk64 = torch.zeros(n, 4, 2, dtype=torch.float64, device=dev)
            for L in torch.unique(ln[due]).tolist():
                rows = torch.nonzero(due & (ln == L)).reshape(-1)
                exact.chunk64[rows] = exact._chain_torch(win[rows, :L].double(), z[rows].double())[0]
            exact.counter.masked_fill_(due, 0)
        c64 = exact.chunk64[torch.arange(n, device=dev), exact.counter.long()]
        exact.counter.add_(1)
        assert torch.equal(fused.counter, plain.counter) and torch.equal(fused.counter, exact.counter), t
        assert torch.equal(fused.hist.len, plain.hist.len) and torch.equal(fused.hist.len, exact.hist.len) and torch.equal(fused.hist.buf, plain.hist.buf), t
        assert torch.equal(fused.last_noise == 0, plain.last_noise == 0), t      # the same entries drawn
        wn = max(wn, float((fused.last_noise - plain.last_noise).abs().max()))
        assert not bool(fused.last_bad.any()) and not bool(plain.last_bad.any())
        worst, yard = max(worst, float((a.double() - c64).abs().max())), max(yard, float((b.double() - c64).abs().max()))
    print("kernel vs f64: %.3e; torch path (f32) vs f64: %.3e; %.2f yardsticks; worst |noise difference| %.3e" % (worst, yard, worst / yard, wn))
    assert worst <= 4 * yard and wn <= 1e-5
    assert fused.counter.tolist() == [(3 if i % 3 == 1 else 1) for i in range(n)] and int(fused._t) == steps == int(plain._t)
    assert fused.hist.len.tolist() == [5] * n


def test_captured_policy_replays_the_kernel_with_fresh_draws(dev, monkeypatch):
    """CapturedPolicy(DDPMACTPolicy) with the runtime's default hardware queues: replay = eager bit for bit over 2 Ta steps starting mid-chunk, fresh noise per chunk,
    warm-up and capture consume neither a step, a window entry nor a chunk position (step word, counters, chunks, window, lengths and last_bad are put back)."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
    n, Ta, T = 64, 4, 16
    obs = (torch.randn(n, 2 * Ta + 1, 10, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.DDPMACTPolicy.random(10, 2, device=dev, seed=5, policy_seed=17, n_envs=n, n_timesteps=T)
    eager, inner = mk(), mk()
    eager.record = inner.record = True
    # the capture happens mid-chunk: one eager step first, on both
    first = inner.predict_batch(obs[:, 0]).clone()
    assert torch.equal(first, eager.predict_batch(obs[:, 0]))
    before = (int(inner._t), inner.counter.clone(), inner.chunk.clone(), inner.hist.buf.clone(), inner.hist.len.clone())
    snap = inner.capture_snapshot(obs[:, 1])
    inner.predict_batch(obs[:, 1])
    inner.capture_restore(snap)      # the hooks by hand: everything is put back
    assert int(inner._t) == before[0] and all(torch.equal(x, y) for x, y in zip((inner.counter, inner.chunk, inner.hist.buf, inner.hist.len), before[1:]))
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    seen = []
    for t in range(1, 2 * Ta + 1):
        if t == Ta + 2:      # an episode restart inside the captured run, in place
            mask = torch.arange(n, device=dev) % 4 == 0
            eager.begin_episodes(mask)
            cap.begin_episodes(mask)
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        if t == 1:      # the first call captured: the state it started from was the state before the capture
            assert int(inner._t) == 2 and inner.counter.tolist() == [2] * n and torch.equal(inner.chunk, before[2]) and inner.hist.len.tolist() == [2] * n
        assert torch.equal(have, want), t
        assert torch.equal(inner.counter, eager.counter) and torch.equal(inner.chunk, eager.chunk) and torch.equal(inner.hist.buf, eager.hist.buf), t
        assert torch.equal(inner.hist.len, eager.hist.len) and torch.equal(inner.last_bad, eager.last_bad) and torch.equal(inner.last_noise, eager.last_noise), t
        assert int(inner._t) == t + 1 == int(eager._t)
        if t % Ta == 0:      # a chunk boundary of the lanes that did not restart: fresh noise, keyed by this step's word
            z = inner.last_noise[1, T].cpu().numpy().copy()
            assert float(np.abs(z - P.ddpm_act_normals(17, 0, n, t, T, Ta, 2)[1]).max()) <= 1e-5 and all(not np.array_equal(z, s) for s in seen)
            seen.append(z)
    assert len(seen) == 2
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    twin = cap.fork()
    assert twin.inner.model is inner.model and twin._g is None and twin.inner.counter is not inner.counter and twin.inner.hist is not inner.hist
    # the torch path decides on the host: it refuses the capture
    monkeypatch.setenv("D3IL_POLICY_DDPM_ACT_FUSED", "0")
    with pytest.raises(RuntimeError):
        mk().captured().predict_batch(obs[:, 0])


def test_a_nan_lane_raises_solver_fail_in_its_avoiding_lane_only(dev, monkeypatch):
    """The policy's NaN action, used as Avoiding_Sim uses a policy output (desired xy = action + previous desired xy), for one env step."""
    from d3il_amd import policies as P
    from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
    monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
    n = 6
    pol = P.DDPMACTPolicy.random(4, 2, device=dev, seed=6, policy_seed=3, n_envs=n, n_timesteps=4)
    obs = (torch.randn(n, 4, generator=torch.Generator().manual_seed(2)) * 0.5).to(dev)
    obs[2, 1] = float("nan")
    act = pol.predict_batch(obs)
    assert pol._packed.key is not None and pol.last_bad.tolist() == [int(r == 2) for r in range(n)]
    assert torch.isnan(act[2]).all() and torch.isfinite(act[[0, 1, 3, 4, 5]]).all()
    env = ObstacleAvoidanceVecEnv(n, device=0)
    try:
        env.start(); env.reset()
        rs = env.robot_state().clone()
        quat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=env.device).expand(n, 4)
        env.step(torch.cat((rs[:, :2] + act.to(torch.float64), rs[:, 2:3], quat), dim=1).contiguous())
        torch.cuda.synchronize()
        fail = (env.flags[:n] & SOLVER_FAIL) != 0
        assert fail.tolist() == [r == 2 for r in range(n)]
    finally:
        env.close()


def _recording_policy(P, dev, obs_dim, A, log):
    """A random-weight DDPMACTPolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, counters, lengths, first-iterate
    noise, actions)."""
    class Rec(P.DDPMACTPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.counter.cpu().numpy().copy(), self.hist.len.cpu().numpy().copy(), self.last_noise[:, self.T].cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.DDPMACTPolicy.random(obs_dim, A, device=dev, seed=6, policy_seed=21, n_timesteps=4)
    base.record = True
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, c, l, z, a in log:
        Cn, Ln, Z, Aa = out.setdefault(t, (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n,) + z.shape[1:], np.float32), np.zeros((n, a.shape[1]), np.float32)))
        Cn[off:off + len(c)], Ln[off:off + len(c)], Z[off:off + len(c)], Aa[off:off + len(c)] = c, l, z, a
    return out


@pytest.mark.parametrize("task", ["avoiding", "sorting"])
def test_sims_give_the_same_actions_and_tables_in_one_and_two_sub_batches(dev, task, monkeypatch):
    """Avoiding_Sim (obs 4 -> 2) and Sorting_Sim (obs 16 -> 2) with a random-weight DDPMACTPolicy, 128 environments, episodes capped at 12 steps, n_sub_batches 1 and
    2: every draw is keyed by the global environment index (set_rollout_range -> env_offset) and rows do not depend on the launch, so the two runs give the same
    actions bit for bit and the same (success, mode) tables."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
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
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(one[t], two[t])), t
    first = min(one)
    assert float(np.abs(one[first][2] - P.ddpm_act_normals(21, 0, n, first, 4, 4, 2)).max()) <= 1e-5 and (one[first][0] == 1).all() and (one[first][1] == 1).all()


def test_as_batched_turns_a_reference_shaped_agent_into_the_policy(dev, monkeypatch):
    """A reference-style enc-dec DiffusionAgent (duck-typed) handed to as_batched runs on DDPMACTPolicy and the kernel, not on RowwiseAgent."""
    from d3il_amd import policies as P
    from d3il_amd.agents import as_batched
    monkeypatch.delenv("D3IL_POLICY_DDPM_ACT_FUSED", raising=False)
    src = P.DDPMACTPolicy.random(10, 2, device=dev, seed=4, n_timesteps=4)
    sc = src.scaler
    diff = types.SimpleNamespace(model=src.model, n_timesteps=4, betas=P.cosine_beta_schedule(4), predict_epsilon=True, clip_denoised=True, diffusion_x=False)
    agent = types.SimpleNamespace(model=diff, scaler=types.SimpleNamespace(x_mean=sc.x_mean, x_std=sc.x_std, y_mean=sc.y_mean, y_std=sc.y_std, y_bounds=sc.y_bounds), obs_seq_len=5,
                                  action_seq_size=4, action_counter=4, window_size=8, diffusion_kde=False, use_ema=False, goal_condition=False, predict=lambda s: None, reset=lambda: None)
    pol = as_batched(agent, 5)
    assert isinstance(pol, P.DDPMACTPolicy) and pol.device.type == "cuda" and pol.counter.tolist() == [4] * 5
    obs = torch.randn(5, 10, generator=torch.Generator().manual_seed(3)).to(dev)
    y = pol.predict_batch(obs)
    assert pol._packed.key is not None and torch.equal(y, src.predict_batch(obs)) and pol.counter.tolist() == [1] * 5
