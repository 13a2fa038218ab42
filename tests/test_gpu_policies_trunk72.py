"""The four native policies with a transformer trunk at the reference's 72-wide shape (n_embd 72, n_head 4, n_layer 4; obs 4 -> 2 actions, the Avoiding width; window
1 or 5): their block chain runs as ONE launch (policies.run_blocks -> d3il_gpt_trunk72_f16x3, csrc/policy_trunk72.h).

Every accuracy comparison is   |kernel-trunk policy - reference| <= 4 x |the same policy under D3IL_POLICY_TRUNK72=0 - reference|   on the same inputs and the same
Philox draws.  The reference of GPTBCPolicy and BeTPolicy is the policy in f64 (trunk and tail).  DDPMGPTPolicy and BESONativePolicy keep their state in f32 by
construction; their reference runs the BLOCK CHAIN in f64 (a double copy of the blocks on torch's layers) inside the same f32 chain and step kernel - the only part
this file's switch changes.  "The kernel path was taken" is a counter around policies.trunk72.  The CPU halves of the input conditions (the BeT margin count) are in
tests/test_policies_trunk72.py::test_the_inputs_do_their_job."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu
SHAPE = dict(n_embd=72, n_layer=4, n_head=4)
OBS, ACT, LANES = 4, 2, 130
U = 2.0 ** -24
BET = dict(seed=3, policy_seed=5, obs_seed=8, steps=5, window=5, margin=1e-4, max_left_out=3)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def defaults(monkeypatch):
    for k in ("D3IL_POLICY_TRUNK72", "D3IL_POLICY_GEMM", "D3IL_POLICY_RANGE_GUARD", "D3IL_POLICY_GPT_BC_HEAD", "D3IL_POLICY_BET_HEAD", "D3IL_POLICY_DDPM_GPT_STEP",
              "D3IL_POLICY_BESO_STEP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("D3IL_POLICY_TRUNK72", "1")      # (whatever the default is: these tests are about the kernel path)


@pytest.fixture
def calls(monkeypatch):
    """Counts the launches of the trunk kernel that go through policies.trunk72."""
    from d3il_amd import policies as P
    seen = []
    real = P.trunk72

    def counted(blocks, x):
        seen.append(tuple(x.shape))
        return real(blocks, x)
    monkeypatch.setattr(P, "trunk72", counted)
    return seen


def observations(seed, n, steps, dev, gain=0.7):
    return (torch.randn(n, steps, OBS, generator=torch.Generator().manual_seed(seed)) * gain).to(dev)


def restart_mask(n, dev):
    m = torch.zeros(n, dtype=torch.bool, device=dev)
    m[5:41] = True
    return m


# ------------------------------------------------------------------------------------------------ 1. GPTBCPolicy
def last_hidden64(ref, s):
    """The f64 trunk of ``ref`` (its trunk is double) on the f32 scaled observation s, at every lane's last token."""
    ref._state(s.shape[0])
    ref.hist.append_(s.float())
    st, ln = ref.hist.padded()
    out = ref.trunk.hidden(st.double())
    return out.gather(1, (ln - 1).view(-1, 1, 1).expand(-1, 1, out.shape[2])).squeeze(1)


@gpu
def test_gpt_bc_policy_takes_the_kernel_and_stays_within_four_yardsticks(dev, calls, monkeypatch):
    """130 lanes x 4 steps, window 5, lanes 5 .. 40 restart at step 2 (the ragged, right-padded path: T = 5 with dead tokens behind a lane's last one)."""
    from d3il_amd import policies as P
    n, T = LANES, 4
    obs = observations(8, n, T, dev)
    mk = lambda: P.GPTBCPolicy.random(OBS, ACT, device=dev, seed=4, window_size=5, head_gain=1.5, bound=1.0, **SHAPE)
    fused, plain, ref = mk(), mk(), mk()
    ref.trunk = ref.trunk.double()
    assert fused.f16x3_blocks
    worst = yard = 0.0
    for t in range(T):
        if t == 2:
            for p in (fused, plain, ref):
                p.begin_episodes(restart_mask(n, dev))
        before = len(calls)
        a = fused.predict_batch(obs[:, t]).clone()
        assert len(calls) == before + 1 and calls[-1][0] == n and calls[-1][2] == 72, "one trunk launch per step"
        monkeypatch.setenv("D3IL_POLICY_TRUNK72", "0")
        assert not plain.f16x3_blocks
        b = plain.predict_batch(obs[:, t]).clone()
        assert len(calls) == before + 1, "the switch gives torch's layers"
        monkeypatch.setenv("D3IL_POLICY_TRUNK72", "1")
        want = ref._tail_torch(last_hidden64(ref, ref.scaler.scale_input(obs[:, t])))
        yard, worst = max(yard, float((b.double() - want).abs().max())), max(worst, float((a.double() - want).abs().max()))
    print("GPTBCPolicy 72 / 4 / 4: kernel trunk %.3e, torch trunk %.3e -> %.2f yardsticks; shapes %s" % (worst, yard, worst / yard, sorted(set(calls))))
    assert sorted(set(fused.hist.padded()[1].tolist())) == [2, 4]      # ragged
    assert not bool(fused.last_bad.any()) and yard > 0 and worst <= 4 * yard


# ------------------------------------------------------------------------------------------------ 2. DDPMGPTPolicy and BESONativePolicy
def with_f64_blocks(pol):
    """``pol`` with its block chain in f64 (a double copy of the blocks, torch's layers), everything else as it is."""
    from d3il_amd import policies as P
    blocks64 = copy.deepcopy(pol.model.blocks).double()
    pol.model.hidden = lambda xbuf, keep: P.run_blocks(blocks64, xbuf.double(), keep=keep).float()
    return pol


def make_sampler(P, kind, dev, window):
    if kind == "ddpm_gpt":
        return P.DDPMGPTPolicy.random(OBS, ACT, device=dev, seed=4, embed_dim=72, n_layers=4, n_heads=4, window_size=window, n_timesteps=8, policy_seed=11)
    return P.BESONativePolicy.random(OBS, ACT, device=dev, seed=4, embed_dim=72, n_layers=4, n_heads=4, window_size=window, num_sampling_steps=16, policy_seed=11)


@gpu
@pytest.mark.parametrize("kind,window", [("ddpm_gpt", 5), ("beso", 5), ("beso", 1)])
def test_samplers_take_the_kernel_and_stay_within_four_yardsticks(dev, kind, window, calls, monkeypatch):
    """130 lanes x 3 steps on the same Philox noise (same policy seed, same step words): the kernel trunk, torch's trunk (the yardstick) and the f64 block chain."""
    from d3il_amd import policies as P
    n, steps = LANES, 3
    obs = observations(9, n, steps, dev, 0.5)
    fused, plain, ref = (make_sampler(P, kind, dev, window) for _ in range(3))
    ref = with_f64_blocks(ref)
    per_call = 8 if kind == "ddpm_gpt" else 16
    assert fused.f16x3_blocks and fused.step_kernel_ok(dev)
    worst = yard = 0.0
    for t in range(steps):
        before = len(calls)
        a = fused.predict_batch(obs[:, t]).clone()
        assert len(calls) == before + per_call and set(calls[before:]) == {(n, 2 * window + 1, 72)}, "every sampling step is one trunk launch"
        monkeypatch.setenv("D3IL_POLICY_TRUNK72", "0")
        b = plain.predict_batch(obs[:, t]).clone()
        want = ref.predict_batch(obs[:, t]).double()
        assert len(calls) == before + per_call
        monkeypatch.setenv("D3IL_POLICY_TRUNK72", "1")
        yard, worst = max(yard, float((b.double() - want).abs().max())), max(worst, float((a.double() - want).abs().max()))
    print("%s window %d: kernel trunk %.3e, torch trunk %.3e -> %.2f yardsticks" % (kind, window, worst, yard, worst / yard))
    assert int(fused.last_bad.sum()) == 0 and yard > 0 and worst <= 4 * yard


@gpu
@pytest.mark.parametrize("kind", ["ddpm_gpt", "beso"])
def test_captured_sampler_equals_eager(dev, kind, calls):
    """CapturedPolicy around the kernel trunk: the replay equals the eager policy bit for bit, step after step, with a restart of two lanes."""
    from d3il_amd import policies as P
    n, steps = 64, 5
    obs = observations(10, n, steps, dev, 0.5)
    eager, inner = make_sampler(P, kind, dev, 5), make_sampler(P, kind, dev, 5)
    cap = P.CapturedPolicy(inner)
    for t in range(steps):
        if t == 3:
            m = torch.zeros(n, dtype=torch.uint8, device=dev)
            m[5:7] = 1
            cap.begin_episodes(m); eager.begin_episodes(m)
        want = eager.predict_batch(obs[:, t]).clone()
        have = cap.predict_batch(obs[:, t]).clone()
        torch.cuda.synchronize()
        assert torch.equal(have, want), t
        assert int(inner._t) == t + 1 == int(eager._t)
    assert cap._g is not None and len(calls) > 0
    g = cap._g
    with P.RangeGuard(dev):      # the guarded instantiation is another kernel: the graph is captured again
        cap.predict_batch(obs[:, 0])
        assert cap._g is not g
    rep_blocks = inner.model.blocks
    assert isinstance(rep_blocks.__dict__.get("_trunk72"), P.PackedWeights) and "_trunk72" not in dict(rep_blocks.named_modules()) and not any("_trunk72" in k for k in inner.model.state_dict())


# ------------------------------------------------------------------------------------------------ 3. BeTPolicy
def bet_policies(P, device):
    """(policy, its f64 twin) at the reference's shape, on ``device``."""
    b = BET
    mk = lambda: P.BeTPolicy.random(OBS, ACT, device=device, seed=b["seed"], window_size=b["window"], policy_seed=b["policy_seed"], **SHAPE)
    pol, ref = mk(), mk()
    ref.trunk = ref.trunk.double()
    pol.record = ref.record = True
    return pol, ref


def bet_reference_step(ref, obs_t):
    """One step of the f64 twin: (logits f64 [n, V], the normalised CDF f64 [n, V], u [n], bins)."""
    ref._tail_torch(last_hidden64(ref, ref.scaler.scale_input(obs_t)))
    ref._t.add_(1)
    return ref.last_logits.double(), torch.cumsum(ref.last_probs.double(), dim=1), ref.last_u.double(), ref.last_bins


def bet_far_lanes(cdf, u):
    return (cdf - u.unsqueeze(1)).abs().min(dim=1).values > BET["margin"]


@gpu
def test_bet_policy_logits_and_bins(dev, calls, monkeypatch):
    """130 lanes x 5 steps, window 5 (the window grows 1 .. 5: T = 1 .. 5 through the trunk kernel), torch's tail (it keeps the logits).  Logits: the bar of the
    four-layer kernel test, 4 x yardstick + (4 + 8 n_layer) 2^-24 max |want|; bins: equal on every lane whose u is farther than 1e-4 from every edge of the f64 CDF."""
    from d3il_amd import policies as P
    b = BET
    n = LANES
    obs = observations(b["obs_seed"], n, b["steps"], dev)
    monkeypatch.setenv("D3IL_POLICY_BET_HEAD", "0")
    fused, ref = bet_policies(P, dev)
    plain, _ = bet_policies(P, dev)
    worst = yard = mag = 0.0
    left_out = []
    for t in range(b["steps"]):
        before = len(calls)
        fused.predict_batch(obs[:, t])
        assert len(calls) == before + 1 and calls[-1] == (n, t + 1, 72)
        monkeypatch.setenv("D3IL_POLICY_TRUNK72", "0")
        plain.predict_batch(obs[:, t])
        monkeypatch.setenv("D3IL_POLICY_TRUNK72", "1")
        logits, cdf, u, bins = bet_reference_step(ref, obs[:, t])
        assert torch.equal(fused.last_u.double(), u) and torch.equal(plain.last_u.double(), u)      # the same Philox uniforms
        worst, yard = max(worst, float((fused.last_logits.double() - logits).abs().max())), max(yard, float((plain.last_logits.double() - logits).abs().max()))
        mag = max(mag, float(logits.abs().max()))
        far = bet_far_lanes(cdf, u)
        left_out.append(int((~far).sum()))
        assert torch.equal(fused.last_bins[far], bins[far]), t
    bound = 4 * yard + (4 + 8 * SHAPE["n_layer"]) * U * mag
    print("BeTPolicy 72 / 4 / 4: logits kernel trunk %.3e, torch trunk %.3e (multiple %.2f, of its bound %.3f); lanes left out of the bin comparison per step %s of %d" % (
        worst, yard, worst / yard, worst / bound, left_out, n))
    assert worst <= bound
    assert max(left_out) <= b["max_left_out"]


# ------------------------------------------------------------------------------------------------ 4. Avoiding_Sim with BESONativePolicy
def _recording_policy(P, dev, log):
    class Rec(P.BESONativePolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, a.cpu().numpy().copy()))
            return a
    base = P.BESONativePolicy.random(OBS, ACT, device=dev, seed=6, embed_dim=72, n_layers=4, n_heads=4, window_size=1, num_sampling_steps=16, policy_seed=21)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


@gpu
def test_avoiding_sim_is_the_same_in_one_and_four_sub_batches(dev, calls):
    """Avoiding_Sim, 64 environments per sub-batch (a sub-batch is at least one wavefront of environments, envs/sub_batch.py MIN_ENVS: 256 is the smallest batch that
    splits in four), episodes capped at 6 steps, BESONativePolicy 72 / 4 / 4 at window 1: the same actions bit for bit and the same (success, mode) tables in one and in
    four sub-batches - a sequence's rows do not depend on the launch they ride in."""
    from d3il_amd import policies as P
    from d3il_amd.simulation.avoiding_sim import Avoiding_Sim
    n, steps = 256, 6
    res = {}
    for nsub in (1, 4):
        log = []
        sim = Avoiding_Sim(seed=0, device="cuda:0", render=False, n_cores=1, n_trajectories=n, max_steps_per_episode=steps, n_sub_batches=nsub)
        sim.test_agent(_recording_policy(P, dev, log))
        r = sim.last_rollout
        tables = (np.asarray(r["counts"]).copy(), r["mode_code"].cpu().numpy(), r["success"].cpu().numpy(), r["n_pos"].cpu().numpy())
        by_step = {}
        for t, off, a in log:
            by_step.setdefault(t, np.zeros((n, ACT), np.float32))[off:off + len(a)] = a
        assert len({off for _, off, _ in log}) == nsub
        res[nsub] = (tables, by_step)
    assert len(calls) > 0 and {c[1:] for c in calls} == {(3, 72)}
    for x, y in zip(res[1][0], res[4][0]):
        assert np.array_equal(x, y)
    one, four = res[1][1], res[4][1]
    assert sorted(one) == sorted(four) and len(one) >= steps
    for t in sorted(one):
        assert np.array_equal(one[t].view(np.uint32), four[t].view(np.uint32)), t
    assert np.isfinite(np.concatenate([one[t] for t in one])).all()
