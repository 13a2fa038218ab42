"""policies.BCGMMPolicy on the GPU: the golden replay of tests/test_policies_bc_gmm.py on cuda:0 (case (a) and (c) through the kernel, (b) through torch's layers with
the warning), the kernel against torch's layers (D3IL_POLICY_BC_GMM_FUSED=0) on the same Philox stream, CapturedPolicy around it, as_batched on a reference-shaped
agent, and Avoiding_Sim in one and in four sub-batches."""
import copy
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_golden_replay_on_the_device(dev, name, monkeypatch):
    from tests.test_policies_bc_gmm import cfg, replay
    monkeypatch.delenv("D3IL_POLICY_BC_GMM_FUSED", raising=False)
    D = cfg(name)["D"]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        worst, pol = replay(name, dev)      # (asserts the golden component on every row)
    said = [w for w in seen if "torch's layers" in str(w.message)]
    print("golden replay %s (device): actions %.3e = %.2f D (D %.3e)" % (name, worst, worst / D, D))
    if name == "b":      # hidden 32: torch's layers, said once
        assert not pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is None and len(said) == 1
    else:
        assert pol.fused_ok(torch.zeros(1, pol.obs_dim, device=dev)) and pol._packed.key is not None and not said      # the kernel ran
    assert worst <= 4 * D
    assert int(pol._t) == 4


def test_kernel_equals_torchs_layers_on_the_same_philox_stream(dev, monkeypatch):
    """257 environments x 2 steps, hidden 256 / 3 blocks, obs 20 -> 3, G 64, exp std: both paths take the same uniform (24 bits, exact in f32); the normals are the
    host's f64 Box-Muller rounded to f32 on the torch path and the device's f32 Box-Muller in the kernel.  EVERY row is compared against the f64 restatement evaluated
    on the draws and at the component that path used; the component against the f64 rule - equal, except that a row whose u sits within BC_GMM_EDGE of an edge of its
    f64 CDF may fall to either side of it.  Bar: 4 x the deviation of torch's f32 layers from f64, measured the same way."""
    from d3il_amd import policies as P
    n, T = 257, 2
    obs = (torch.randn(n, T, 20, generator=torch.Generator().manual_seed(8)) * 0.7).to(dev)
    mk = lambda: P.BCGMMPolicy.random(20, 3, device=dev, seed=4, hidden_dim=256, n_blocks=3, n_gaussians=64, policy_seed=(7 << 32) + 13, low_noise_eval=False, bound=0.5)
    fused, plain = mk(), mk()
    fused.record = plain.record = True
    ref = copy.copy(plain)
    ref.model = copy.deepcopy(plain.model).double()

    def at_component(s64, k, z):      # the f64 restatement with the component forced: a u in the middle of that component's share of the CDF
        p = ref._predict_torch(s64, torch.full((n,), 0.5, device=dev, dtype=torch.float64), z.double())[2]
        c = torch.cumsum(p, dim=1)
        mid = (c - 0.5 * p)[torch.arange(n, device=dev), k.long()]
        y, kk, _ = ref._predict_torch(s64, mid, z.double())
        assert torch.equal(kk, k)
        return y, c

    worst = yard = 0.0
    near_rows = split_rows = 0
    for t in range(T):
        monkeypatch.delenv("D3IL_POLICY_BC_GMM_FUSED", raising=False)
        a = fused.predict_batch(obs[:, t])
        assert fused._packed.key is not None
        monkeypatch.setenv("D3IL_POLICY_BC_GMM_FUSED", "0")
        b = plain.predict_batch(obs[:, t])
        assert plain._packed.key is None
        u_host = torch.as_tensor(P.bc_gmm_uniforms((7 << 32) + 13, 0, n, t)).to(dev)
        assert torch.equal(plain.last_u, u_host) and torch.equal(fused.last_u, u_host)      # bit for bit
        assert float((fused.last_z - plain.last_z).abs().max()) < 1e-5
        s64 = ref.scaler.scale_input(obs[:, t]).double()
        ya, cdf = at_component(s64, fused.last_comps, fused.last_z)
        yb, _ = at_component(s64, plain.last_comps, plain.last_z)
        k64 = (cdf <= u_host.double().unsqueeze(1)).sum(dim=1).clamp_max(63).to(torch.int32)
        near = (cdf - u_host.double().unsqueeze(1)).abs().min(dim=1).values < P.BC_GMM_EDGE
        near_rows += int(near.sum())
        for pol in (fused, plain):
            assert (pol.last_comps >= 0).all() and torch.equal(pol.last_comps[~near], k64[~near])
            assert bool(((pol.last_comps[near] - k64[near]).abs() <= 1).all())
        split_rows += int((fused.last_comps != plain.last_comps).sum())
        yard = max(yard, float((b.double() - yb).abs().max()))
        worst = max(worst, float((a.double() - ya).abs().max()))
    print("kernel against f64: actions %.3e, torch f32 %.3e -> %.2f yardsticks; rows within EDGE of a CDF edge: %d of %d, rows on which the two f32 paths drew different "
          "components: %d" % (worst, yard, worst / yard, near_rows, n * T, split_rows))
    assert yard > 0 and worst <= 4 * yard
    assert int(fused._t) == T == int(plain._t)


def test_captured_policy_replays_the_kernel_with_fresh_draws(dev, monkeypatch):
    """CapturedPolicy(BCGMMPolicy) with the machine's default hardware queues: replay = eager bit for bit over 5 steps, fresh draws per replay, the step word advances
    once per step (warm-up and capture do not count); the torch path refuses the capture."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_BC_GMM_FUSED", raising=False)
    n, T = 64, 5
    obs = (torch.randn(n, T, 4, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.BCGMMPolicy.random(4, 2, device=dev, seed=5, hidden_dim=128, n_blocks=3, n_gaussians=8, policy_seed=17, low_noise_eval=False)
    eager, inner = mk(), mk()
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    seen = []
    for t in range(T):
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        assert torch.equal(have, want), t
        assert torch.equal(inner.last_comps, eager.last_comps) and torch.equal(inner.last_u, eager.last_u) and torch.equal(inner.last_z, eager.last_z), t
        assert np.array_equal(inner.last_u.cpu().numpy(), P.bc_gmm_uniforms(17, 0, n, t)), t
        u, z = inner.last_u.cpu().numpy().copy(), inner.last_z.cpu().numpy().copy()
        assert all(not np.array_equal(u, s[0]) and not np.array_equal(z, s[1]) for s in seen)
        seen.append((u, z))
        assert int(inner._t) == t + 1 == int(eager._t)
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    # torch's layers take their Philox numbers from the host: that path refuses the capture
    monkeypatch.setenv("D3IL_POLICY_BC_GMM_FUSED", "0")
    with pytest.raises(RuntimeError):
        mk().captured().predict_batch(obs[:, 0])


def test_as_batched_on_the_device(dev, monkeypatch):
    """A reference-shaped BC_GMM_Agent whose model lives on the device becomes a BCGMMPolicy there and replays step 0 of golden case (a) through the kernel."""
    from d3il_amd import policies as P
    from d3il_amd.agents import as_batched
    from tests.test_policies_bc_gmm import BC_GMM_Agent, Bank, G, cfg
    monkeypatch.delenv("D3IL_POLICY_BC_GMM_FUSED", raising=False)
    agent = BC_GMM_Agent()
    agent.model.to(dev)
    pol = as_batched(agent, 6)
    assert isinstance(pol, P.BCGMMPolicy) and pol.device.type == "cuda" and next(pol.model.parameters()).is_cuda
    b = Bank("a")
    pol.u_in, pol.z_in = b.u, b.z
    a = pol.predict_batch(torch.as_tensor(G["gm_a_obs"][:, 0], device=dev)).cpu().numpy().astype(np.float64)
    assert pol._packed.key is not None
    assert np.array_equal(pol.last_comps.cpu().numpy(), G["gm_a_comps"][:, 0]) and float(np.abs(a - G["gm_a_ref64"][:, 0]).max()) <= 4 * cfg("a")["D"]


def _recording_policy(P, dev, log):
    """A random-weight BCGMMPolicy (Avoiding's shape, low_noise_eval off) whose predict_batch - and that of its forks, which share ``log`` - appends (step word,
    env_offset, u, z, components, actions)."""
    class Rec(P.BCGMMPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, self.last_u.cpu().numpy().copy(), self.last_z.cpu().numpy().copy(), self.last_comps.cpu().numpy().copy(), a.cpu().numpy().copy()))
            return a
    base = P.BCGMMPolicy.random(4, 2, device=dev, seed=6, hidden_dim=128, n_blocks=3, n_gaussians=8, policy_seed=21, low_noise_eval=False, action_scale=0.004)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def test_avoiding_sim_gives_the_same_draws_actions_and_tables_in_one_and_four_sub_batches(dev, monkeypatch):
    """Avoiding_Sim (obs 4 -> 2) with BCGMMPolicy.random, 256 trajectories, episodes capped at 25 steps, n_sub_batches 1 and 4: every draw is keyed by the global
    environment index (set_rollout_range -> env_offset) and rows do not depend on the launch, so the two runs give the same uniforms, normals, components and actions
    bit for bit and the same (success, mode) tables.  No lane is marked and every recorded position is finite: the sim keeps no flag word, and a lane whose
    solver flag a NaN action raises stops moving with NaN in its desired position."""
    from d3il_amd import policies as P
    from d3il_amd.simulation.avoiding_sim import Avoiding_Sim
    monkeypatch.delenv("D3IL_POLICY_BC_GMM_FUSED", raising=False)
    n, steps = 256, 25
    res = {}
    for nsub in (1, 4):
        log = []
        sim = Avoiding_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_trajectories=n, max_steps_per_episode=steps, n_sub_batches=nsub)
        sim.test_agent(_recording_policy(P, dev, log))
        r = sim.last_rollout
        tables = (np.asarray(r["counts"]).copy(), r["mode_code"].cpu().numpy(), r["success"].cpu().numpy(), r["n_pos"].cpu().numpy())
        assert bool(torch.isfinite(r["c_pos"]).all())
        assert len({off for _, off, *_ in log}) == nsub and r["success"].shape[0] == n
        by = {}
        for t, off, u, z, k, a in log:
            U, Z, K, Aa = by.setdefault(t, (np.zeros(n, np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)))
            U[off:off + len(u)], Z[off:off + len(u)], K[off:off + len(u)], Aa[off:off + len(u)] = u, z, k, a
        res[nsub] = (tables, by)
    for x, y in zip(res[1][0], res[4][0]):
        assert np.array_equal(x, y)
    one, four = res[1][1], res[4][1]
    assert sorted(one) == sorted(four) and len(one) >= steps
    for t in sorted(one):
        assert np.array_equal(one[t][0], P.bc_gmm_uniforms(21, 0, n, t)), t
        for x, y in zip(one[t], four[t]):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), t
        assert (one[t][2] >= 0).all() and (one[t][2] < 8).all()      # no lane is marked: every action is finite
    assert np.isfinite(np.concatenate([one[t][3] for t in one])).all()
    assert len(np.unique(np.concatenate([one[t][2] for t in one]))) == 8
