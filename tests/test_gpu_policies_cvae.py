"""policies.CVAEPolicy on the GPU: the golden replay of tests/test_policies_cvae.py on cuda:0 through the decode kernel, the kernel against torch's layers
(D3IL_POLICY_CVAE_FUSED=0) on the same Philox stream, CapturedPolicy around it, and Avoiding_Sim / Sorting_Sim in one and in two sub-batches."""
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
    from tests.test_policies_cvae import D, replay
    monkeypatch.delenv("D3IL_POLICY_CVAE_FUSED", raising=False)
    worst, pol = replay(dev)
    print("golden replay (kernel): actions %.3e = %.2f D (D %.3e)" % (worst, worst / D, D))
    assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None      # the kernel ran, not torch's layers
    assert worst <= 4 * D
    assert int(pol._t) == 4


def test_kernel_equals_torchs_layers_on_the_same_philox_stream(dev, monkeypatch):
    """130 environments x 4 steps, hidden 256 / 4 blocks, obs 20 -> 8, latent 16: both paths draw the same latent (the kernel's Box-Muller in f32, the host's in f64);
    there is no discrete choice, so every row is compared.  Bar: 4 x the deviation of torch's f32 layers from the same decoder in f64 on the same rows."""
    from d3il_amd import policies as P
    n, T = 130, 4
    obs = (torch.randn(n, T, 20, generator=torch.Generator().manual_seed(8)) * 0.7).to(dev)
    mk = lambda: P.CVAEPolicy.random(20, 8, device=dev, seed=4, hidden_dim=256, n_blocks=4, latent_dim=16, policy_seed=13, weight_gain=1.6)
    fused, plain = mk(), mk()
    ref = copy.copy(plain)
    ref.model = copy.deepcopy(plain.model).double()
    worst = yard = zdiff = 0.0
    for t in range(T):
        monkeypatch.delenv("D3IL_POLICY_CVAE_FUSED", raising=False)
        a = fused.predict_batch(obs[:, t])
        assert fused._packed.key is not None
        monkeypatch.setenv("D3IL_POLICY_CVAE_FUSED", "0")
        b = plain.predict_batch(obs[:, t])
        assert plain._packed.key is None
        z_host = torch.as_tensor(P.cvae_latent_normals(13, 0, n, t, 16), dtype=torch.float32).to(dev)
        assert torch.equal(plain.last_z, z_host.clamp(-0.5, 0.5))
        zdiff = max(zdiff, float((fused.last_z - plain.last_z).abs().max()))
        want, _ = ref._decode_torch(ref.scaler.scale_input(obs[:, t]).double(), z_host.double())
        yard = max(yard, float((b.double() - want).abs().max()))
        worst = max(worst, float((a - b).abs().max()))
    print("kernel vs torch's layers: worst |a - b| %.3e, torch f32 against f64 %.3e -> %.2f yardsticks; latents differ by at most %.3e" % (worst, yard, worst / yard, zdiff))
    assert zdiff < 1e-5      # the kernel's f32 Box-Muller against the host's f64 one
    assert yard > 0 and worst <= 4 * yard
    assert int(fused._t) == T == int(plain._t)


def test_captured_policy_replays_the_kernel_with_fresh_draws(dev, monkeypatch):
    """CapturedPolicy(CVAEPolicy) with the runtime's default hardware queues: replay = eager bit for bit, fresh draws per replay, the step word advances once per step
    (warm-up and capture do not count)."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_CVAE_FUSED", raising=False)
    n, T = 64, 5
    obs = (torch.randn(n, T, 4, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.CVAEPolicy.random(4, 2, device=dev, seed=5, hidden_dim=128, n_blocks=3, latent_dim=32, policy_seed=17)
    eager, inner = mk(), mk()
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    seen = []
    for t in range(T):
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        assert torch.equal(have, want), t
        assert torch.equal(inner.last_z, eager.last_z), t
        host = np.clip(P.cvae_latent_normals(17, 0, n, t, 32), -0.5, 0.5)
        assert float(np.abs(inner.last_z.double().cpu().numpy() - host).max()) < 1e-5, t
        z = inner.last_z.cpu().numpy().copy()
        assert all(not np.array_equal(z, s) for s in seen)
        seen.append(z)
        assert int(inner._t) == t + 1 == int(eager._t)
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    twin = cap.fork()
    assert twin.inner.model is inner.model and twin._g is None
    # torch's layers take their Philox numbers from the host: that path refuses the capture
    monkeypatch.setenv("D3IL_POLICY_CVAE_FUSED", "0")
    with pytest.raises(RuntimeError):
        mk().captured().predict_batch(obs[:, 0])


def _recording_policy(P, dev, obs_dim, A, log):
    """A random-weight CVAEPolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, latent, actions)."""
    class Rec(P.CVAEPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.last_z.cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.CVAEPolicy.random(obs_dim, A, device=dev, seed=6, hidden_dim=128, n_blocks=3, latent_dim=16, policy_seed=21)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, z, a in log:
        Z, Aa = out.setdefault(t, (np.zeros((n, z.shape[1]), np.float32), np.zeros((n, a.shape[1]), np.float32)))
        Z[off:off + len(z)], Aa[off:off + len(z)] = z, a
    return out


@pytest.mark.parametrize("task", ["avoiding", "sorting"])
def test_sims_give_the_same_actions_and_tables_in_one_and_two_sub_batches(dev, task, monkeypatch):
    """Avoiding_Sim (obs 4 -> 2) and Sorting_Sim (obs 16 -> 2) with a random-weight CVAEPolicy, 128 environments, episodes capped at 12 steps, n_sub_batches 1 and 2:
    every draw is keyed by the global environment index (set_rollout_range -> env_offset) and rows do not depend on the launch, so the two runs give the same
    latents and actions bit for bit and the same (success, mode) tables."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_CVAE_FUSED", raising=False)
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
        host = np.clip(P.cvae_latent_normals(21, 0, n, t, 16), -0.5, 0.5)
        assert float(np.abs(one[t][0].astype(np.float64) - host).max()) < 1e-5, t
        assert np.array_equal(one[t][0].view(np.uint32), two[t][0].view(np.uint32)) and np.array_equal(one[t][1].view(np.uint32), two[t][1].view(np.uint32)), t
    assert np.isfinite(np.concatenate([one[t][1] for t in one])).all()
