"""policies.GPTBCPolicy on the GPU: the golden replay of tests/test_policies_gpt_bc.py on cuda:0 (torch trunk + head kernel), the head kernel against torch's tail
(D3IL_POLICY_GPT_BC_HEAD=0) behind the same trunk, CapturedPolicy around it, and Avoiding_Sim / Sorting_Sim in one and in two sub-batches."""
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
    from tests.test_policies_gpt_bc import D, T_STEPS, replay
    monkeypatch.delenv("D3IL_POLICY_GPT_BC_HEAD", raising=False)
    worst, pol = replay(dev)
    print("golden replay (kernel): actions %.3e = %.2f D (D %.3e)" % (worst, worst / D, D))
    assert pol.head_kernel_ok(torch.zeros(1, pol.trunk.n_embd, device=dev))      # the kernel ran, not torch's tail
    assert worst <= 4 * D
    assert int(pol._t) == T_STEPS


def _with_hidden(P, pol):
    """``pol`` recording the hidden rows its tail is handed (``seen_h``)."""
    class Rec(type(pol)):
        def tail(self, h):
            self.seen_h = h.clone()
            return super().tail(h)
    rec = Rec.__new__(Rec)
    rec.__dict__.update(pol.__dict__)
    return rec


@pytest.mark.parametrize("n_embd", [72, 120])
def test_kernel_equals_torchs_tail_behind_the_same_trunk(dev, n_embd, monkeypatch):
    """130 environments x 4 steps, window 5, 6 heads, obs 20 -> 8; lanes 5 .. 40 restart at step 2, so steps 2 and 3 run the ragged, right-padded path.  Both
    policies run the same trunk (72 wide: torch's layers; 120 wide: the matrix-core kernels) and get the same hidden rows bit for bit; every row's action is compared
    with the f64 tail on those rows.  Bar: 4 x the deviation of torch's f32 tail from f64."""
    from d3il_amd import policies as P
    n, T = 130, 4
    obs = (torch.randn(n, T, 20, generator=torch.Generator().manual_seed(8)) * 0.7).to(dev)
    mk = lambda: _with_hidden(P, P.GPTBCPolicy.random(20, 8, device=dev, seed=4, n_embd=n_embd, n_layer=2, n_head=6, window_size=5, head_gain=1.5, bound=1.0))
    fused, plain = mk(), mk()
    ref = copy.copy(plain)
    ref.trunk = copy.deepcopy(plain.trunk).double()
    worst = yard = 0.0
    clamped = total = 0
    for t in range(T):
        if t == 2:
            m = torch.zeros(n, dtype=torch.bool, device=dev)
            m[5:41] = True
            fused.begin_episodes(m); plain.begin_episodes(m)
        monkeypatch.delenv("D3IL_POLICY_GPT_BC_HEAD", raising=False)
        a = fused.predict_batch(obs[:, t])
        assert fused.last_bad.dtype == torch.int32 and not bool(fused.last_bad.any())
        monkeypatch.setenv("D3IL_POLICY_GPT_BC_HEAD", "0")
        b = plain.predict_batch(obs[:, t])
        assert torch.equal(fused.seen_h, plain.seen_h), t      # the same trunk, the same rows
        h64 = plain.seen_h.double()
        want = ref._tail_torch(h64)
        o = torch.nn.functional.linear(ref.trunk.ln_f(h64), ref.trunk.head.weight)
        clamped, total = clamped + int(((o < -1.0) | (o > 1.0)).sum()), total + o.numel()
        yard = max(yard, float((b.double() - want).abs().max()))
        worst = max(worst, float((a.double() - want).abs().max()))
    print("n_embd %d: kernel %.3e, torch f32 %.3e -> %.2f yardsticks; %d of %d outputs clamped; window lengths at the end %s" % (
        n_embd, worst, yard, worst / yard, clamped, total, sorted(set(fused.hist.padded()[1].tolist()))))
    assert 0 < clamped < total
    assert sorted(set(fused.hist.padded()[1].tolist())) == [2, 4]      # ragged
    assert yard > 0 and worst <= 4 * yard
    assert int(fused._t) == T == int(plain._t)


def test_captured_policy_replays_the_chain(dev, monkeypatch):
    """CapturedPolicy(GPTBCPolicy) with the runtime's default hardware queues, 120 wide (matrix-core trunk + head kernel), 5 steps with a restart of two lanes: the
    replay equals, bit for bit, both the uncaptured policy on the same fixed-shape chain (right-padded windows, what a capture runs) and the plain eager policy
    (lockstep windows) - the rows of the matrix-core trunk do not depend on the launch.  It also stays within 4 yardsticks of the policy in f64, the yardstick being
    the deviation of the plain eager policy from that f64 run.  The step word advances once per step (warm-up and capture do not count).  There are no draws, and
    torch's tail is a chain of device kernels too: nothing here refuses a capture."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_GPT_BC_HEAD", raising=False)
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    n, T = 64, 5
    obs = (torch.randn(n, T, 20, generator=torch.Generator().manual_seed(9)) * 0.7).to(dev)
    mk = lambda: P.GPTBCPolicy.random(20, 8, device=dev, seed=5, n_embd=120, n_layer=2, n_head=6, window_size=5)
    eager, fixed, inner = mk(), mk(), mk()
    fixed._static = True
    ref = mk()
    ref.trunk = ref.trunk.double()
    cap = inner.captured()
    assert isinstance(cap, P.CapturedPolicy)
    worst = yard = 0.0
    for t in range(T):
        if t == 3:
            m = torch.zeros(n, dtype=torch.uint8, device=dev); m[5:7] = 1
            for p in (cap, eager, fixed, ref):
                p.begin_episodes(m)
        plain = eager.predict_batch(obs[:, t]).clone()
        want = fixed.predict_batch(obs[:, t]).clone()
        r64 = ref.scaler.scale_input(obs[:, t]).double()
        ref._state(n); ref.hist.append_(r64.float())
        st, ln = ref.hist.padded()
        out = ref.trunk.hidden(st.double())
        exact = ref._tail_torch(out.gather(1, (ln - 1).view(-1, 1, 1).expand(-1, 1, out.shape[2])).squeeze(1))
        have = cap.predict_batch(obs[:, t])
        torch.cuda.synchronize()
        assert torch.equal(have, want), t
        assert torch.equal(have, plain), t      # ... and the plain eager policy (lockstep windows, only the last token through the last block)
        yard = max(yard, float((plain.double() - exact).abs().max()))
        worst = max(worst, float((have.double() - exact).abs().max()))
        assert int(inner._t) == t + 1 == int(eager._t)
    print("captured against f64: %.3e, eager %.3e -> %.2f yardsticks" % (worst, yard, worst / yard))
    assert yard > 0 and worst <= 4 * yard
    g = cap._g
    cap.predict_batch(obs[:, 0])
    assert cap._g is g      # a replay, not another capture
    assert inner.hist.len.tolist() == [3 if 5 <= e < 7 else 5 for e in range(n)]      # (lanes 5 and 6 restarted at step 3: steps 3 and 4 and the extra replay)
    twin = cap.fork()
    assert twin.inner.trunk is inner.trunk and twin.inner.hist is None and twin._g is None


def _recording_policy(P, dev, obs_dim, A, log):
    """A random-weight GPTBCPolicy whose predict_batch - and that of its forks, which share ``log`` - appends (step word, env_offset, actions)."""
    class Rec(P.GPTBCPolicy):
        def predict_batch(self, obs):
            t = int(self._t)
            a = super().predict_batch(obs)
            log.append((t, self.env_offset, a.cpu().numpy().copy()))
            return a
    base = P.GPTBCPolicy.random(obs_dim, A, device=dev, seed=6, n_embd=120, n_layer=2, n_head=6, window_size=5)
    pol = Rec.__new__(Rec)
    pol.__dict__.update(base.__dict__)
    return pol


def _by_step(log, n):
    out = {}
    for t, off, a in log:
        Aa = out.setdefault(t, np.zeros((n, a.shape[1]), np.float32))
        Aa[off:off + len(a)] = a
    return out


@pytest.mark.parametrize("task", ["avoiding", "sorting"])
def test_sims_give_the_same_actions_and_tables_in_one_and_two_sub_batches(dev, task, monkeypatch):
    """Avoiding_Sim (obs 4 -> 2) and Sorting_Sim (obs 16 -> 2) with a random-weight GPTBCPolicy (120 wide: the matrix-core trunk, whose rows do not depend on the
    launch), 128 environments, episodes capped at 12 steps, n_sub_batches 1 and 2: the same actions bit for bit and the same (success, mode) tables."""
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_GPT_BC_HEAD", raising=False)
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
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
        assert np.array_equal(one[t].view(np.uint32), two[t].view(np.uint32)), t
    assert np.isfinite(np.concatenate([one[t] for t in one])).all()
