"""policies.DDPMNativePolicy on the GPU: the golden replay of tests/test_policies_ddpm_mlp.py on cuda:0 (case a through the chain kernel, b and c on torch's
layers), the kernel against the policy's own torch path (D3IL_POLICY_DDPM_MLP_CHAIN=0) on the same Philox stream, CapturedPolicy around it, a reference-shaped
agent through as_batched, and Sorting_Sim in one and in four sub-batches - identical actions and tables, the property the older DDPMPolicy cannot have."""
import copy
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAG_BAD = (1 << 16) | (1 << 18)      # solver failure, contact overflow
SWITCH = "D3IL_POLICY_DDPM_MLP_CHAIN"


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("c", ["a", "b", "c"])
def test_golden_replay_on_the_device(dev, c, monkeypatch):
    from tests.test_policies_ddpm_mlp import G, replay
    monkeypatch.delenv(SWITCH, raising=False)
    D = float(G[c + "_D"])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        w64, w32, pol, _ = replay(c, dev)
    fallback = [w for w in caught if "not one the chain kernel is built for" in str(w.message)]
    print("golden replay (cuda), case %s: D %.3e, worst |action - f64 reference| %.3e (%.2f D), worst |action - f32 reference| %.3e" % (c, D, w64, w64 / D, w32))
    assert w64 <= 4 * D
    assert int(pol._t) == 8 and pol.last_bad.tolist() == [0] * 6
    if c == "a":      # a kernel shape: the kernel ran, not torch's layers
        assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None and not fallback
    else:             # hidden 32: torch's layers, with the warning once per policy
        assert not pol._kernel_shape() and pol._packed.key is None and len(fallback) == 1


@pytest.mark.parametrize("hidden, n_blocks, obs, A, t_dim, T", [(128, 3, 20, 3, 8, 4), (256, 4, 16, 2, 8, 4), (256, 4, 20, 8, 4, 4)])
def test_kernel_against_the_torch_path_on_the_same_philox_stream(dev, hidden, n_blocks, obs, A, t_dim, T, monkeypatch):
    """257 environments x 3 steps: both paths draw the same Philox numbers (the kernel in f32 on the device, the torch path in f64 on the host, rounded to f32: equal
    to Box-Muller accuracy), and each is held against the f64 NumPy chain of tests/test_gpu_ddpm_mlp_chain.py on the noise IT recorded.  Bar: the kernel within 4 x the
    deviation of the torch path.  Bounds of +-10, for the reason that file's docstring gives."""
    from d3il_amd import policies as P
    from tests.test_gpu_ddpm_mlp_chain import chain64
    n, steps = 257, 3
    states = (torch.randn(n, steps, obs, generator=torch.Generator().manual_seed(8)) * 0.8).to(dev)
    mk = lambda: P.DDPMNativePolicy.random(obs, A, device=dev, seed=4, hidden_dim=hidden, n_blocks=n_blocks, t_dim=t_dim, n_timesteps=T, policy_seed=(5 << 32) | 13, bound=10.0)
    fused, plain = mk(), mk()
    for p in (fused, plain):
        p.record = True
        p.set_rollout_range(1000, n)
        with torch.no_grad():
            p.model.layers.layers[-1].weight.mul_(4.0)
    worst = yard = 0.0
    for t in range(steps):
        monkeypatch.delenv(SWITCH, raising=False)
        a = fused.predict_batch(states[:, t])
        assert fused._packed.key is not None
        monkeypatch.setenv(SWITCH, "0")
        b = plain.predict_batch(states[:, t])
        assert plain._packed.key is None
        host = np.stack([P.ddpm_mlp_normals((5 << 32) | 13, 1000, n, t, k, A) for k in range(T)])
        assert tuple(fused.last_noise.shape) == tuple(plain.last_noise.shape) == (T + 1, n, A) and not fused.last_noise[T].any() and not plain.last_noise[T].any()
        assert np.array_equal(plain.last_noise[:T].cpu().numpy(), host.astype(np.float32))
        assert float(np.abs(fused.last_noise[:T].double().cpu().numpy() - host).max()) < 4e-6
        assert not fused.last_bad.any() and not plain.last_bad.any()
        w = fused._packed.buf
        s = fused.scaler.scale_input(states[:, t])
        want_a, _ = chain64(fused, w["temb"], w["sched"], s, fused.last_noise)
        want_b, _ = chain64(plain, w["temb"], w["sched"], s, plain.last_noise)
        worst = max(worst, float(np.abs(a.double().cpu().numpy() - want_a).max()))
        yard = max(yard, float(np.abs(b.double().cpu().numpy() - want_b).max()))
    print("hidden %d, %d blocks, A %d: kernel %.3e, torch path %.3e -> %.2f yardsticks" % (hidden, n_blocks, A, worst, yard, worst / yard))
    assert yard > 0 and worst <= 4 * yard
    assert int(fused._t) == steps == int(plain._t)


def test_captured_policy_replays_the_kernel_with_fresh_draws(dev, monkeypatch):
    """CapturedPolicy(DDPMNativePolicy) with the runtime's default hardware queues: replay = eager bit for bit over 5 steps, fresh draws per replay, the step word
    advances once per step (warm-up and capture do not count); the torch path refuses the capture."""
    from d3il_amd import policies as P
    monkeypatch.delenv(SWITCH, raising=False)
    n, steps = 64, 5
    obs = (torch.randn(n, steps, 16, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.DDPMNativePolicy.random(16, 2, device=dev, seed=5, policy_seed=17)
    eager, inner = mk(), mk()
    eager.record = inner.record = True
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    seen = []
    for t in range(steps):
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        assert torch.equal(have, want), t
        assert torch.equal(inner.last_noise, eager.last_noise) and torch.equal(inner.last_bad, eager.last_bad), t
        z = inner.last_noise.cpu().numpy().copy()
        assert float(np.abs(z[0].astype(np.float64) - P.ddpm_mlp_normals(17, 0, n, t, 0, 2)).max()) < 4e-6, t
        assert all(not np.array_equal(z, s) for s in seen)
        seen.append(z)
        assert int(inner._t) == t + 1 == int(eager._t)
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    twin = cap.fork()
    assert twin.inner.model is inner.model and twin._g is None
    # torch's layers take their Philox numbers from the host: that path refuses the capture
    monkeypatch.setenv(SWITCH, "0")
    with pytest.raises(RuntimeError):
        mk().captured().predict_batch(obs[:, 0])


def test_as_batched_gives_the_native_policy_and_runs_the_kernel(dev, monkeypatch):
    from d3il_amd import policies as P
    from d3il_amd.agents import as_batched
    from tests.test_policies_ddpm_mlp import Bank, G, _stand_in_agent
    monkeypatch.delenv(SWITCH, raising=False)
    agent = _stand_in_agent("a")
    agent.model.model.to(dev)
    pol = as_batched(agent, 6)
    assert isinstance(pol, P.DDPMNativePolicy) and pol.device.type == "cuda" and pol.model is not agent.model.model
    pol.noise_in = Bank(G["a_noise"][:, :, :, -1])
    for t in range(3):
        a = pol.predict_batch(torch.as_tensor(G["a_obs"][:, t], device=dev))
        assert float(np.abs(a.double().cpu().numpy() - G["a_ref64"][:, t]).max()) <= 4 * float(G["a_D"])
    assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None and int(pol._t) == 3


def _recording_policy(P, dev, log):
    """The random-weight policy of the config-4 shape (obs 16 -> 2, hidden 256, 8 hidden layers, t_dim 8, T 4) whose predict_batch - and that of its forks, which
    share ``log`` - appends (step word, env_offset, first draw, bad, actions)."""
    class Rec(P.DDPMNativePolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.last_noise[0].cpu().numpy().copy(), self.last_bad.cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.DDPMNativePolicy.random(16, 2, device=dev, seed=6, hidden_dim=256, n_blocks=4, t_dim=8, n_timesteps=4, policy_seed=21)
    base.record = True
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, z, b, a in log:
        Z, B, Aa = out.setdefault(t, (np.zeros((n, z.shape[1]), np.float32), np.zeros(n, np.int32), np.zeros((n, a.shape[1]), np.float32)))
        Z[off:off + len(z)], B[off:off + len(z)], Aa[off:off + len(z)] = z, b, a
    return out


def test_sorting_sim_gives_the_same_actions_and_tables_in_one_and_four_sub_batches(dev, monkeypatch):
    """Sorting_Sim (obs 16 -> 2) with the config-4 shape, 256 environments, episodes capped at 12 steps, n_sub_batches 1 and 4: every draw is keyed by the global
    environment index (set_rollout_range -> env_offset) and rows do not depend on the launch, so the two runs give the same draws and actions bit for bit and the
    same (success, mode) tables, without a solver flag."""
    from d3il_amd import policies as P
    from d3il_amd.simulation.sorting_sim import Sorting_Sim
    monkeypatch.delenv(SWITCH, raising=False)
    n, steps = 256, 12
    res = {}
    for nsub in (1, 4):
        log = []
        sim = Sorting_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_contexts=16, n_trajectories_per_context=16, max_steps_per_episode=steps, n_sub_batches=nsub)
        pol = _recording_policy(P, dev, log)
        sim.test_agent(pol)
        assert pol.fused_ok(torch.zeros(1, 16, device=dev))
        r = sim.last_rollout
        tables = (np.asarray(r["counts"]).copy(), r["mode"].cpu().numpy(), r["success"].cpu().numpy())
        assert not bool((r["flags"] & FLAG_BAD).any())
        offsets = sorted({off for _, off, *_ in log})
        assert offsets == [0, 64, 128, 192][:nsub] if nsub == 4 else offsets == [0]      # the batch is really cut: four sub-batches of a wavefront each
        assert r["success"].shape[0] == n
        res[nsub] = (tables, _by_step(log, n))
    for x, y in zip(res[1][0], res[4][0]):
        assert np.array_equal(x, y)
    one, four = res[1][1], res[4][1]
    assert sorted(one) == sorted(four) and len(one) >= steps
    for t in sorted(one):
        assert float(np.abs(one[t][0].astype(np.float64) - P.ddpm_mlp_normals(21, 0, n, t, 0, 2)).max()) < 4e-6, t
        assert np.array_equal(one[t][0].view(np.uint32), four[t][0].view(np.uint32)) and np.array_equal(one[t][1], four[t][1]), t
        assert np.array_equal(one[t][2].view(np.uint32), four[t][2].view(np.uint32)), t
        assert not one[t][1].any()
    assert np.isfinite(np.concatenate([one[t][2] for t in one])).all()
