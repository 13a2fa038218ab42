"""Option "quiet_streams" of the step group (d3il_group_set_option).

With the option on, the caller declares that between two merged rounds it queues nothing on the members' streams (the first member's excepted) that touches
what the step touches; the library then joins the other members' streams before the launch only in an ARMED round (the first one, and the first after a
flush, any other library call on a member, a member leaving, another `actions` buffer, a switch of the option) and lets every other round follow the previous
one on the first member's stream.  The waits AFTER the launch stay in every round.

Members, episode length, step count, snapshots and the golden `collide` drive are those of tests/test_gpu_avoiding_step_group.py (the file of the default
mode, which this one imports): 64, 64, 40 and 1 environments, 12-step episodes, 40 steps; everything is compared bit for bit (np.array_equal) with the same
handles ungrouped.  d3il_group_stats (merged rounds, rounds that joined) shows which form a round took.

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
CHILD_S = 4.4


def _quiet_set(serve_max_wg=256):
    s = base.Set(True, serve_max_wg)
    s.group.set_option("quiet_streams", 1)
    return s


def _device_snapshots(s):
    return [None if m is None else m.device_snapshot() for m in s.members]


def _run_pair(serve_max_wg, collide):
    from d3il_amd import capi
    g, u = _quiet_set(serve_max_wg), base.Set(False, serve_max_wg)
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
            g.group.flush()      # the override is written on member 2's stream before the round: the caller's re-arming point
        g.step(t, override); u.step(t, override)
        if collide:
            m = u.members[2]
            with torch.cuda.stream(m.stream):
                touched |= ((m.env.flags[:m.n] & capi.FLAG_ROD_CONTACT) != 0).any()
                retired_next |= touched & (m.env.last_reset != 0).any()
        if t in (0, 1, 13):      # device copies behind a device synchronisation, no library call: the rounds of g keep continuing
            base._equal(_device_snapshots(g), _device_snapshots(u), t)
    merged, joined = g.group.stats()
    assert merged == STEPS - 1      # (step 0 is the first call of every sequence: single launches)
    assert joined == (merged if collide else 1), (merged, joined)
    snaps = g.snapshots()
    base._equal(snaps, u.snapshots(), "end")
    for sn, n in zip(snaps, SIZES):
        assert int(sn["episodes"][0]) == int(sn["tally"][:, 0].sum()) >= 3 * n
    if collide:
        assert bool(touched) and bool(retired_next)
    g.close(); u.close()


@pytest.mark.parametrize("serve_max_wg", [256, 0])
def test_quiet_group_equals_ungrouped(serve_max_wg):
    _run_pair(serve_max_wg, collide=False)


def test_quiet_group_equals_ungrouped_with_a_member_in_contact():
    _run_pair(256, collide=True)


def _next_merged_round_joins(g, t):
    """Steps until a round merges (a call that was not eligible costs its own round): that round joined, the one after it continues.  Returns the next t."""
    m0, j0 = g.group.stats()
    for _ in range(2):
        g.step(t); t += 1
        if g.group.stats()[0] > m0:
            break
    assert g.group.stats() == (m0 + 1, j0 + 1), (g.group.stats(), m0, j0)
    g.step(t); t += 1
    assert g.group.stats() == (m0 + 2, j0 + 1), (g.group.stats(), m0, j0)
    return t


def test_counters_and_what_arms_a_round():
    g = _quiet_set()
    g.step(0)
    assert g.group.stats() == (0, 0)
    t = 1
    for _ in range(40):
        g.step(t); t += 1
    assert g.group.stats() == (40, 1)
    g.group.flush()      # nothing pending: arms all the same
    t = _next_merged_round_joins(g, t)
    g.members[1].env.get_state()
    t = _next_merged_round_joins(g, t)
    g.members[2].env.set_option("serve_wave_max_workgroups", 256)
    t = _next_merged_round_joins(g, t)
    m3 = g.members[3]
    with torch.cuda.stream(m3.stream):
        m3.actions = torch.zeros_like(m3.actions)      # another `actions` buffer: the member's call starts a new sequence on its own
    m3.stream.synchronize()
    t = _next_merged_round_joins(g, t)
    g.close_member(3)
    t = _next_merged_round_joins(g, t)
    g.group.set_option("quiet_streams", 0)
    m0, j0 = g.group.stats()
    for _ in range(3):
        g.step(t); t += 1
    assert g.group.stats() == (m0 + 3, j0 + 3)      # option off: every merged round joins
    g.group.set_option("quiet_streams", 1)
    t = _next_merged_round_joins(g, t)
    g.close()
    d = base.Set(True)      # a group that never heard of the option
    for k in range(5):
        d.step(k)
    assert d.group.stats() == (4, 4)
    d.close()


def test_readers_on_other_streams_stay_ordered_behind_a_continuing_round():
    """The first member's stream is kept busy, so the continuing round's dispatch starts late; clones queued on two other members' streams right after the
    round, without a host synchronisation, must still see it (the post-launch waits are kept)."""
    g, u = _quiet_set(), base.Set(False)
    clones = []
    for s in (g, u):
        for t in range(3):
            s.step(t)
        torch.cuda.synchronize()
        with torch.cuda.stream(s.members[0].stream):
            torch.cuda._sleep(10_000_000)
        s.step(3)
        got = []
        for m in (s.members[1], s.members[3]):
            with torch.cuda.stream(m.stream):
                got.append((m.env.obs.clone(), m.env.last_reset.clone(), m.env.step_count[:m.n].clone()))
        clones.append(got)
    assert g.group.stats() == (3, 1)      # round 3 continued round 2: no join
    torch.cuda.synchronize()
    for (ga, gb, gc), (ua, ub, uc) in zip(*clones):
        assert torch.equal(ga, ua) and torch.equal(gb, ub) and torch.equal(gc, uc)
    base._equal(g.snapshots(), u.snapshots(), "readers")
    g.close(); u.close()


def test_flush_orders_a_write_on_another_stream_again():
    """The delayed-write pattern of the default mode's file: member 1's stream sleeps, then writes its step counters; group.flush() before the round re-arms the
    join, so the round sees the write and all of member 1 times out."""
    g, u = _quiet_set(), base.Set(False)
    clones = []
    for s in (g, u):
        for t in range(3):
            s.step(t)
        torch.cuda.synchronize()
        m1 = s.members[1]
        with torch.cuda.stream(s.members[0].stream):
            torch.cuda._sleep(10_000_000)
        with torch.cuda.stream(m1.stream):
            torch.cuda._sleep(20_000_000)
            m1.env.step_count[:m1.n] = MAX_STEPS - 1
        if s.group is not None:
            s.group.flush()
        s.step(3)
        got = []
        for m in (s.members[1], s.members[3]):
            with torch.cuda.stream(m.stream):
                got.append((m.env.obs.clone(), m.env.last_reset.clone(), m.env.step_count[:m.n].clone()))
        clones.append(got)
    assert g.group.stats() == (3, 2)
    torch.cuda.synchronize()
    for (ga, gb, gc), (ua, ub, uc) in zip(*clones):
        assert torch.equal(ga, ua) and torch.equal(gb, ub) and torch.equal(gc, uc)
    assert bool(clones[0][0][1].all())      # the write was seen: all of member 1 was reset by that step
    base._equal(g.snapshots(), u.snapshots(), "re-armed")
    g.close(); u.close()


def test_timing_with_quiet_streams():
    from d3il_amd import capi
    g = _quiet_set()
    g.step(0)
    for m in g.members:
        m.env.set_timing(True)
    rounds = 6
    for t in range(1, 1 + rounds):
        g.step(t)
    assert g.group.stats() == (rounds, 1)      # set_timing armed the first of them; the end event of the timed pair is what the other streams wait for
    last = [m.env.last_step_ms() for m in g.members]
    stats = [m.env.timing_stats() for m in g.members]
    assert all(s[3] == rounds for s in stats), stats      # one launch per member and step
    assert all(s == stats[0] for s in stats) and 0.0 < stats[0][1] <= stats[0][2] <= stats[0][0], stats
    assert all(x == last[0] for x in last) and last[0] > 0.0, last
    for t in range(1 + rounds, 3 + rounds):
        g.step(t)
    g.group.close(); g.group = None      # the shared pairs die with the group: the durations are kept, the last launch is no longer there to report
    for m in g.members:
        with pytest.raises(capi.D3ilError, match="no step recorded"):
            m.env.last_step_ms()
    stats = [m.env.timing_stats() for m in g.members]
    assert all(s[3] == rounds + 2 for s in stats), stats
    g.step(3 + rounds)      # ungrouped: every member launches on its own, with its own event pair
    assert all(m.env.last_step_ms() > 0.0 for m in g.members)
    assert all(m.env.timing_stats()[3] == rounds + 3 for m in g.members)
    g.close()


def test_this_file_passes_on_the_poison_build():
    """-DD3IL_POISON: the LDS of the group forms starts as NaN; the quiet rounds run the same kernels."""
    if os.environ.get("D3IL_LIB_PATH"):
        pytest.skip("already running on a variant library")
    if not os.path.exists(POISON):
        pytest.fail("libd3il_rollout_poison.so not built (python -c 'from d3il_amd import build; build.build_poison()')")
    env = dict(os.environ, D3IL_LIB_PATH=POISON)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "tests/test_gpu_avoiding_group_quiet.py"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=3 * CHILD_S)
    print("poison child: %.1f s" % (time.perf_counter() - t0))
    assert r.returncode == 0, "\n".join(r.stdout.splitlines()[-15:])
