"""policies.ACTPolicy on the GPU: the golden replay of tests/test_policies_act.py on cuda:0 through the chunk kernel, the kernel against the torch path
(D3IL_POLICY_ACT_FUSED=0) on the same Philox stream, CapturedPolicy around it, and Avoiding_Sim / Sorting_Sim in one and in two sub-batches."""
import copy
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAG_BAD = (1 << 16) | (1 << 18)      # solver failure, contact overflow


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_golden_replay_through_the_kernel(dev, monkeypatch):
    from tests.test_policies_act import D, replay
    monkeypatch.delenv("D3IL_POLICY_ACT_FUSED", raising=False)
    wa, wc, same, exact, n_edge, pol = replay(dev)
    print("golden replay (kernel): actions %.3e = %.2f D, chunks %.3e = %.2f D (D %.3e); %d chunk entries on a clamp bound" % (wa, wa / D, wc, wc / D, D, n_edge))
    assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None      # the kernel ran, not the torch path
    assert same and exact and n_edge > 0
    assert wa <= 4 * D and wc <= 4 * D
    assert int(pol._t) == 7


def test_kernel_equals_the_torch_path_on_the_same_philox_stream(dev, monkeypatch):
    """130 environments x 7 steps of the shipped shape, a begin_episodes mask at step 2: both paths draw the same latents and keep the same counters; the chunks
    are deterministic given the latent, so no row is left out.  Yardstick: the deviation of the torch path (f32) from the same path in f64, taken here; bar 4 of them."""
    from d3il_amd import policies as P
    n, steps = 130, 7
    obs = (torch.randn(n, steps, 10, generator=torch.Generator().manual_seed(8)) * 0.7).to(dev)
    mk = lambda: P.ACTPolicy.random(10, 2, 3, device=dev, seed=4, policy_seed=13, n_envs=n)
    fused, plain, exact = mk(), mk(), mk()
    exact.model = copy.deepcopy(exact.model).double()
    mask = (torch.arange(n, device=dev) % 3 == 1)
    worst = yard = 0.0
    for t in range(steps):
        if t == 2:
            for p in (fused, plain, exact):
                p.begin_episodes(mask)
        monkeypatch.delenv("D3IL_POLICY_ACT_FUSED", raising=False)
        a = fused.predict_batch(obs[:, t])
        assert fused._packed.key is not None
        monkeypatch.setenv("D3IL_POLICY_ACT_FUSED", "0")
        b = plain.predict_batch(obs[:, t])
        # the f64 table of the same step: the torch path on a double network (its bookkeeping is the policy's own)
        due = exact.counter >= exact.T
        if bool(due.any()):
            z = torch.as_tensor(P.act_latent_uniforms(13, 0, n, t)).to(dev)
            s = exact.scaler.scale_input(obs[:, t]).double()
            exact.chunk64 = torch.where(due.reshape(-1, 1, 1), exact._chunk_torch(s, z.double()), getattr(exact, "chunk64", torch.zeros(n, 3, 2, dtype=torch.float64, device=dev)))
            exact.counter.masked_fill_(due, 0)
        c64 = exact.chunk64[torch.arange(n, device=dev), exact.counter.long()]
        exact.counter.add_(1)
        exact._t.add_(1)
        assert torch.equal(fused.counter, plain.counter) and torch.equal(fused.counter, exact.counter), t
        assert torch.equal(fused.last_latent, plain.last_latent), t
        worst, yard = max(worst, float((a.double() - c64).abs().max())), max(yard, float((b.double() - c64).abs().max()))
    print("kernel vs f64: %.3e; torch path (f32) vs f64: %.3e; %.2f yardsticks" % (worst, yard, worst / yard))
    assert worst <= 4 * yard
    assert fused.counter.tolist() == [(2 if i % 3 == 1 else 1) for i in range(n)] and int(fused._t) == steps == int(plain._t)
    assert np.array_equal(fused.last_latent[0].cpu().numpy(), P.act_latent_uniforms(13, 0, n, 6)[0]) and np.array_equal(fused.last_latent[1].cpu().numpy(), P.act_latent_uniforms(13, 0, n, 5)[1])


def test_captured_policy_replays_the_kernel_with_fresh_draws(dev, monkeypatch):
    """CapturedPolicy(ACTPolicy) with the runtime's default hardware queues: replay = eager bit for bit over 2 T steps, a fresh latent per chunk, warm-up and
    capture consume neither a step nor a chunk position (step word, counters and chunks are put back)."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_ACT_FUSED", raising=False)
    n, T = 64, 3
    obs = (torch.randn(n, 2 * T + 1, 10, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.ACTPolicy.random(10, 2, T, device=dev, seed=5, policy_seed=17, n_envs=n)
    eager, inner = mk(), mk()
    # the capture happens mid-chunk: one eager step first, on both
    first = inner.predict_batch(obs[:, 0]).clone()
    assert torch.equal(first, eager.predict_batch(obs[:, 0]))
    before = (int(inner._t), inner.counter.clone(), inner.chunk.clone())
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    seen = []
    for t in range(1, 2 * T + 1):
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        if t == 1:      # the first call captured: the state it started from was the state before the capture
            assert before[0] == 1 and int(inner._t) == 2 and inner.counter.tolist() == [2] * n and torch.equal(inner.chunk, before[2])
        assert torch.equal(have, want), t
        assert torch.equal(inner.counter, eager.counter) and torch.equal(inner.chunk, eager.chunk) and torch.equal(inner.last_latent, eager.last_latent), t
        assert int(inner._t) == t + 1 == int(eager._t)
        if t % T == 0:      # a chunk boundary: a fresh draw, keyed by this step's word
            z = inner.last_latent.cpu().numpy().copy()
            assert np.array_equal(z, P.act_latent_uniforms(17, 0, n, t)) and all(not np.array_equal(z, s) for s in seen)
            seen.append(z)
    assert len(seen) == 2
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    twin = cap.fork()
    assert twin.inner.model is inner.model and twin._g is None and twin.inner.counter is not inner.counter
    # the torch path decides on the host: it refuses the capture
    monkeypatch.setenv("D3IL_POLICY_ACT_FUSED", "0")
    with pytest.raises(RuntimeError):
        mk().captured().predict_batch(obs[:, 0])


def _recording_policy(P, dev, obs_dim, A, log):
    """A random-weight ACTPolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, counters, latents, actions)."""
    class Rec(P.ACTPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.counter.cpu().numpy().copy(), self.last_latent.cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.ACTPolicy.random(obs_dim, A, 3, device=dev, seed=6, policy_seed=21)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, c, z, a in log:
        Cn, Z, Aa = out.setdefault(t, (np.zeros(n, np.int64), np.zeros((n, 32), np.float32), np.zeros((n, a.shape[1]), np.float32)))
        Cn[off:off + len(c)], Z[off:off + len(c)], Aa[off:off + len(c)] = c, z, a
    return out


@pytest.mark.parametrize("task", ["avoiding", "sorting"])
def test_sims_give_the_same_actions_and_tables_in_one_and_two_sub_batches(dev, task, monkeypatch):
    """Avoiding_Sim (obs 4 -> 2) and Sorting_Sim (obs 16 -> 2) with a random-weight ACTPolicy, 128 environments, episodes capped at 12 steps, n_sub_batches 1 and 2:
    every draw is keyed by the global environment index (set_rollout_range -> env_offset) and rows do not depend on the launch, so the two runs give the same
    actions bit for bit and the same (success, mode) tables."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_ACT_FUSED", raising=False)
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
        if t % 3 == 0:
            assert np.array_equal(one[t][1], P.act_latent_uniforms(21, 0, n, t)), t
        assert np.array_equal(one[t][0], two[t][0]) and np.array_equal(one[t][1], two[t][1]) and np.array_equal(one[t][2].view(np.uint32), two[t][2].view(np.uint32)), t
        assert (one[t][0] == t % 3 + 1).all()


def test_as_batched_turns_a_reference_shaped_agent_into_the_policy(dev, monkeypatch):
    from d3il_amd import policies as P
    from d3il_amd.agents import as_batched
    monkeypatch.delenv("D3IL_POLICY_ACT_FUSED", raising=False)
    src = P.ACTPolicy.random(10, 2, 3, device=dev, seed=4)
    sc = src.scaler
    agent = types.SimpleNamespace(model=src.model, scaler=types.SimpleNamespace(x_mean=sc.x_mean, x_std=sc.x_std, y_mean=sc.y_mean, y_std=sc.y_std, y_bounds=sc.y_bounds), gc=False,
                                  obs_size=1, window_size=3, action_seq_size=3, action_counter=3, predict=lambda s: None, reset=lambda: None)
    pol = as_batched(agent, 5)
    assert isinstance(pol, P.ACTPolicy) and pol.device.type == "cuda" and pol.counter.tolist() == [3] * 5
    obs = torch.randn(5, 10, generator=torch.Generator().manual_seed(3)).to(dev)
    y = pol.predict_batch(obs)
    assert pol._packed.key is not None and torch.equal(y, src.predict_batch(obs)) and pol.counter.tolist() == [1] * 5
