"""Option "dispatch_sets" of the step group (d3il_group_set_option).

With K = 2 the four members form two dispatch sets, members 0 and 1 (leader: member 0) and members 2 and 3 (leader: member 2).  A set launches when all ITS
members have called, as one dispatch on its leader's stream, and does not wait for the other set: the sets may be steps apart.  Whatever ends a round ends
the pending rounds of both sets.  d3il_group_stats counts merged DISPATCHES: two per step when both sets merge.

Members, episode length, step count, snapshots and the golden `collide` drive are those of tests/test_gpu_avoiding_step_group.py (which this file imports,
the way tests/test_gpu_avoiding_group_quiet.py does): 64, 64, 40 and 1 environments, 12-step episodes, 40 steps.  Set 0 is two whole workgroups, set 1 a
partial last workgroup (first workgroup index 0 inside the set, 24 dead lanes) and a one-lane member at workgroup 1.  Everything is compared bit for bit
(np.array_equal) with the same handles ungrouped.  The sets run with "quiet_streams" 1, as d3il_amd/envs/sub_batch.py runs them.

Poison build: the whole file passes in a child process on libd3il_rollout_poison.so.  CHILD_S: the child's wall time measured on one MI355X, process start
included; its limit is three times that."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from tests import test_gpu_avoiding_step_group as base      # noqa: E402  (Member, Set, the snapshots and the contact drive; a module, so nothing of it is collected here)

ROOT = base.ROOT
POISON = base.POISON
SIZES, MAX_STEPS, STEPS = base.SIZES, base.MAX_STEPS, base.STEPS
CHILD_S = 4.2


def _sets_group(serve_max_wg=256, k=2):
    s = base.Set(True, serve_max_wg)
    s.group.set_option("quiet_streams", 1)
    s.group.set_option("dispatch_sets", k)
    return s


def _device_snapshots(s, only=None):
    return [None if (m is None or (only is not None and i not in only)) else m.device_snapshot() for i, m in enumerate(s.members)]


def _run_pair(serve_max_wg, collide):
    from d3il_amd import capi
    g, u = _sets_group(serve_max_wg), base.Set(False, serve_max_wg)
    override = None
    if collide:
        for s in (g, u):
            base._drive_member_to_contact(s, 2)
        dev = torch.device("cuda:0")
        rows = [torch.as_tensor(np.repeat(base.COL[min(base.COL_FROM + t, len(base.COL) - 1)][None], SIZES[2], 0), dtype=torch.float64, device=dev) for t in range(STEPS)]
        override = lambda i, t: rows[t] if (i == 2 and t > 0) else None
    touched = torch.zeros((), dtype=torch.bool, device="cuda:0")
    retired_next = torch.zeros((), dtype=torch.bool, device="cuda:0")
    for t in range(STEPS):
        if collide:
            g.group.flush()      # the override is written on member 2's stream before the round: the caller's re-arming point (arms both sets)
        g.step(t, override); u.step(t, override)
        if collide:
            m = u.members[2]
            with torch.cuda.stream(m.stream):
                touched |= ((m.env.flags[:m.n] & capi.FLAG_ROD_CONTACT) != 0).any()
                retired_next |= touched & (m.env.last_reset != 0).any()
        if t in (0, 1, 13):      # device copies behind a device synchronisation, no library call: the rounds of both sets keep continuing
            base._equal(_device_snapshots(g), _device_snapshots(u), t)
    merged, joined = g.group.stats()
    assert merged == 2 * (STEPS - 1)      # (step 0 is the first call of every sequence: single launches); one dispatch per set and step
    assert joined == (merged if collide else 2), (merged, joined)      # each set's first round joins, the others continue
    snaps = g.snapshots()
    base._equal(snaps, u.snapshots(), "end")
    for sn, n in zip(snaps, SIZES):
        assert int(sn["episodes"][0]) == int(sn["tally"][:, 0].sum()) >= 3 * n
    if collide:
        assert bool(touched) and bool(retired_next)
    g.close(); u.close()


@pytest.mark.parametrize("serve_max_wg", [256, 0])
def test_two_sets_equal_ungrouped(serve_max_wg):
    _run_pair(serve_max_wg, collide=False)


def test_two_sets_equal_ungrouped_with_a_member_in_contact():
    """Member 2, the leader of the second set, on the golden `collide` set-points: its lanes take the rod contact inside the set's dispatch."""
    _run_pair(256, collide=True)


def test_a_set_runs_ahead_of_the_other():
    """Members 0 and 1 step five times while members 2 and 3 are not called at all: every step is one merged dispatch of the first set, and what it left
    is on the device without any call on the second set.  Then the second set catches up on its own."""
    g, u = _sets_group(), base.Set(False)
    g.step(0); u.step(0)
    assert g.group.stats() == (0, 0)
    idle = _device_snapshots(g, only=(2, 3))
    for t in range(1, 6):
        for s in (g, u):
            s.members[0].call(t); s.members[1].call(t)
        assert g.group.stats() == (t, 1), (t, g.group.stats())      # one dispatch per step; only the first joined
        base._equal(_device_snapshots(g, only=(0, 1)), _device_snapshots(u, only=(0, 1)), ("ahead", t))
    base._equal(_device_snapshots(g, only=(2, 3)), idle, "the second set has not moved")
    for t in range(1, 6):
        before = _device_snapshots(g, only=(2, 3))
        for s in (g, u):
            s.members[2].call(t)
        base._equal(_device_snapshots(g, only=(2, 3)), before, ("half a round of the second set", t))
        for s in (g, u):
            s.members[3].call(t)
        assert g.group.stats() == (5 + t, 2), (t, g.group.stats())
        base._equal(_device_snapshots(g), _device_snapshots(u), ("catching up", t))
    for t in range(6, 10):      # together again, still two dispatches per step, still no join
        g.step(t); u.step(t)
    assert g.group.stats() == (10 + 2 * 4, 2)
    base._equal(g.snapshots(), u.snapshots(), "end")
    g.close(); u.close()


def test_round_keys_are_per_set_and_end_through_the_single_path():
    g, u = _sets_group(), base.Set(False)
    for t in range(3):
        g.step(t); u.step(t)
    m0 = g.group.stats()[0]
    # a second call of member 0 before member 1's call: with the next t (not eligible while the first is deferred), then with the same t (a pending member)
    for s in (g, u):
        s.members[0].call(3); s.members[0].call(4)
        s.members[1].call(3); s.members[1].call(4)
        for t in (3, 4):
            s.members[2].call(t); s.members[3].call(t)
    assert g.group.stats()[0] == m0 + 2      # the second set merged both of its rounds, the first set none
    base._equal(g.snapshots(), u.snapshots(), "second call, next t")
    for s in (g, u):
        s.members[0].call(5); s.members[0].call(5)
        s.members[1].call(5)
        s.members[2].call(5); s.members[3].call(5)
    base._equal(g.snapshots(), u.snapshots(), "second call, same t")
    # a jump of t (the first call of a new sequence: not eligible), then every member on a t of its own: eligible calls that fit no round of their set
    for k in range(3):
        for s in (g, u):
            for i, m in enumerate(s.members):
                m.call(100 * (i + 1) + k)
    base._equal(g.snapshots(), u.snapshots(), "different t")
    # members of one set on a common t, the sets 50 steps apart: both merge
    for s in (g, u):
        for i, m in enumerate(s.members):
            m.call(1000 + 50 * (i // 2))
    m1 = g.group.stats()[0]
    for k in (1, 2):
        for s in (g, u):
            for i, m in enumerate(s.members):
                m.call(1000 + 50 * (i // 2) + k)
    assert g.group.stats()[0] == m1 + 4
    base._equal(g.snapshots(), u.snapshots(), "sets apart")
    g.close(); u.close()


def test_readers_behind_a_busy_leader_of_the_second_set():
    """Member 2's stream (the leader of the second set) is kept busy, so the set's continuing dispatch starts late; clones queued on member 3's stream right
    after the round, without a host synchronisation, must still see it (the post-launch waits inside the set are kept)."""
    g, u = _sets_group(), base.Set(False)
    clones = []
    for s in (g, u):
        for t in range(3):
            s.step(t)
        torch.cuda.synchronize()
        with torch.cuda.stream(s.members[2].stream):
            torch.cuda._sleep(10_000_000)
        s.step(3)
        got = []
        for m in (s.members[3], s.members[1]):
            with torch.cuda.stream(m.stream):
                got.append((m.env.obs.clone(), m.env.last_reset.clone(), m.env.step_count[:m.n].clone()))
        clones.append(got)
    assert g.group.stats() == (6, 2)      # round 3 continued round 2 in both sets: no join
    torch.cuda.synchronize()
    for (ga, gb, gc), (ua, ub, uc) in zip(*clones):
        assert torch.equal(ga, ua) and torch.equal(gb, ub) and torch.equal(gc, uc)
    base._equal(g.snapshots(), u.snapshots(), "readers")
    g.close(); u.close()


def test_flush_orders_a_write_on_member_3_before_the_leaders_dispatch():
    """Member 3's stream sleeps, then writes its step counter; the leader's stream is busy too.  group.flush() before the round re-arms the join of the set,
    so the round sees the write and member 3 times out."""
    g, u = _sets_group(), base.Set(False)
    clones = []
    for s in (g, u):
        for t in range(3):
            s.step(t)
        torch.cuda.synchronize()
        m3 = s.members[3]
        with torch.cuda.stream(s.members[2].stream):
            torch.cuda._sleep(10_000_000)
        with torch.cuda.stream(m3.stream):
            torch.cuda._sleep(20_000_000)
            m3.env.step_count[:m3.n] = MAX_STEPS - 1
        if s.group is not None:
            s.group.flush()
        s.step(3)
        got = []
        for m in (s.members[3], s.members[2]):
            with torch.cuda.stream(m.stream):
                got.append((m.env.obs.clone(), m.env.last_reset.clone(), m.env.step_count[:m.n].clone()))
        clones.append(got)
    assert g.group.stats() == (6, 4)      # the flush armed both sets
    torch.cuda.synchronize()
    for (ga, gb, gc), (ua, ub, uc) in zip(*clones):
        assert torch.equal(ga, ua) and torch.equal(gb, ub) and torch.equal(gc, uc)
    assert bool(clones[0][0][1].all())      # the write was seen: member 3 was reset by that step
    base._equal(g.snapshots(), u.snapshots(), "re-armed")
    g.close(); u.close()


def test_timing_is_per_set():
    from d3il_amd import capi
    g = _sets_group()
    g.step(0)
    for m in g.members:
        m.env.set_timing(True)
    rounds = 6
    for t in range(1, 1 + rounds):
        g.step(t)
    assert g.group.stats() == (2 * rounds, 2)
    last = [m.env.last_step_ms() for m in g.members]
    stats = [m.env.timing_stats() for m in g.members]
    assert all(s[3] == rounds for s in stats), stats      # one launch per member and step
    assert all(0.0 < s[1] <= s[2] <= s[0] for s in stats), stats      # every duration is positive
    assert all(x > 0.0 for x in last) and last[0] == last[1] and last[2] == last[3], last      # the pair of a set is shared by its members
    assert stats[0] == stats[1] and stats[2] == stats[3], stats
    for t in range(1 + rounds, 3 + rounds):
        g.step(t)
    g.group.close(); g.group = None      # the shared pairs die with the group - the durations are kept, the last launch is no longer there to report
    for m in g.members:
        with pytest.raises(capi.D3ilError, match="no step recorded"):
            m.env.last_step_ms()
    stats = [m.env.timing_stats() for m in g.members]
    assert all(s[3] == rounds + 2 for s in stats), stats
    g.step(3 + rounds)      # ungrouped: every member launches on its own, with its own event pair
    assert all(m.env.last_step_ms() > 0.0 for m in g.members)
    assert all(m.env.timing_stats()[3] == rounds + 3 for m in g.members)
    g.close()


def test_option_values_a_set_of_one_and_back_to_one_set():
    from d3il_amd import capi
    g, u = _sets_group(), base.Set(False)
    for bad in (0, 5):
        with pytest.raises(capi.D3ilError, match="error -1: dispatch_sets"):      # D3IL_EINVAL
            g.group.set_option("dispatch_sets", bad)
    for t in range(3):
        g.step(t); u.step(t)
    assert g.group.stats()[0] == 4
    for s in (g, u):
        s.close_member(3)      # the second set is member 2 alone: it still launches the group form, on its own
    with pytest.raises(capi.D3ilError, match="error -1: dispatch_sets"):
        g.group.set_option("dispatch_sets", 4)      # three live members
    m0 = g.group.stats()[0]
    for t in range(3, 7):
        g.step(t); u.step(t)
    assert g.group.stats()[0] == m0 + 2 * 4
    base._equal(_device_snapshots(g), _device_snapshots(u), "a set of one")
    before = g.members[2].device_snapshot()
    g.members[2].call(7)      # nobody else has called: the one-member set has launched all the same
    assert base._changed([before], [g.members[2].device_snapshot()])[0]
    g.members[0].call(7); g.members[1].call(7)
    u.step(7)
    base._equal(g.snapshots(), u.snapshots(), 7)
    g.group.set_option("dispatch_sets", 1)      # mid-sequence: one dispatch per step again
    m0 = g.group.stats()[0]
    for t in range(8, 12):
        g.step(t); u.step(t)
    assert g.group.stats()[0] == m0 + 4
    base._equal(g.snapshots(), u.snapshots(), "one set again")
    g.close(); u.close()


def test_this_file_passes_on_the_poison_build():
    """-DD3IL_POISON: the LDS of the group forms starts as NaN; the dispatches of a set run the same kernels."""
    if os.environ.get("D3IL_LIB_PATH"):
        pytest.skip("already running on a variant library")
    if not os.path.exists(POISON):
        pytest.fail("libd3il_rollout_poison.so not built (python -c 'from d3il_amd import build; build.build_poison()')")
    env = dict(os.environ, D3IL_LIB_PATH=POISON)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "tests/test_gpu_avoiding_group_sets.py"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=3 * CHILD_S)
    print("poison child: %.1f s" % (time.perf_counter() - t0))
    assert r.returncode == 0, "\n".join(r.stdout.splitlines()[-15:])
