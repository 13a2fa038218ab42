"""Option "pipeline_depth" of the step group (d3il_group_set_option).

With D = 2 or 3 consecutive merged rounds overlap: round r of a running sequence launches on the r mod D-th of the first D member streams with no event
between the rounds, and every workgroup of round r waits on the device for its own predecessor of round r - 1 (one epoch word per workgroup, agent-scope
release / acquire).  Whatever arms a round (d3il_group_flush, any other library call on a member, an option switch, a member leaving) ends the sequence:
every member stream then waits for the last round of every launch stream.  d3il_group_pipeline_stats counts the pipelined rounds and the give-ups reported.

Members, episode length, step count, snapshots and the golden `collide` drive are those of tests/test_gpu_avoiding_step_group.py (which this file imports,
the way tests/test_gpu_avoiding_group_quiet.py does): 64, 64, 40 and 1 environments on four streams, 12-step episodes, 40 steps; four workgroups per round.
Everything is compared bit for bit (np.array_equal) with the same handles ungrouped - at the end through the API, and at steps 0, 1 and 13 behind a device
synchronisation with no library call, so the sequence keeps running across the comparison.

The `collide` case writes member 2's set-points over the drawn action before every round.  That write is the caller's, on a member stream, so it needs the
re-arming point (flush) before every round, as in the sibling files: every round then STARTS a sequence (the pipelined form with nothing to wait for,
behind the join, the zeroed epoch words and the start event) and ENDS one - 39 times with a rod contact inside the dispatch.  Rounds that really run ahead of
a slower workgroup are what the warm-consumer cases below produce.

Warm consumer: a hand-off that forgets its acquire passes on an idle chip with cold L1s.  Before every round a plain torch kernel reads every member's state
rows on the launch streams (the lines are then in some CU's L1 in whatever version was there), once on an otherwise idle chip and once beside unrelated
matrix products on the null stream (uneven progress of the rounds).

No test here makes a workgroup wait for an epoch that never comes: the give-up decision is one small device function (pipe_give_up, csrc/rollout.hip),
reviewed by reading.  Every run ends with a fault counter of 0.

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
CHILD_S = 4.8


def _pipe_group(depth, serve_max_wg=256):
    s = base.Set(True, serve_max_wg)
    s.group.set_option("quiet_streams", 1)
    s.group.set_option("pipeline_depth", depth)
    return s


def _device_snapshots(s):
    return [None if m is None else m.device_snapshot() for m in s.members]


def _finish(g, u, where="end"):
    """the end of every run: equal through the API (get_state reads the group's fault word), no give-up counted, then the group's destruction reads it again"""
    base._equal(g.snapshots(), u.snapshots(), where)
    assert g.group.pipeline_stats()[1] == 0
    g.close(); u.close()


def _run_pair(depth, serve_max_wg=256, collide=False, warm=False, busy=False):
    from d3il_amd import capi
    g, u = _pipe_group(depth, serve_max_wg), base.Set(False, serve_max_wg)
    override = None
    dev = torch.device("cuda:0")
    if collide:
        for s in (g, u):
            base._drive_member_to_contact(s, 2)
        rows = [torch.as_tensor(np.repeat(base.COL[min(base.COL_FROM + t, len(base.COL) - 1)][None], SIZES[2], 0), dtype=torch.float64, device=dev) for t in range(STEPS)]
        override = lambda i, t: rows[t] if (i == 2 and t > 0) else None
    touched = torch.zeros((), dtype=torch.bool, device=dev)
    sinks = [torch.zeros((), dtype=torch.float64, device=dev) for _ in g.members]
    load = torch.ones(768, 768, device=dev) if busy else None
    for t in range(STEPS):
        if collide:
            g.group.flush()      # the override is written on member 2's stream before the round: the caller's re-arming point
        if warm:      # plain loads of every member's state rows on the launch streams: stale or not, the lines are in an L1 when the round starts
            for k in range(depth):
                with torch.cuda.stream(g.members[k].stream):
                    for m in g.members:
                        sinks[k] += m.env.state[:, :m.n].sum() + m.env.flags[:m.n].sum() + m.actions.sum()
        if busy:
            for _ in range(3):
                load = (load @ load) * (1.0 / 768.0)
        g.step(t, override); u.step(t, override)
        if collide:
            m = u.members[2]
            with torch.cuda.stream(m.stream):
                touched |= ((m.env.flags[:m.n] & capi.FLAG_ROD_CONTACT) != 0).any()
        if t in (0, 1, 13):      # device copies behind a device synchronisation, no library call: the sequence keeps running
            base._equal(_device_snapshots(g), _device_snapshots(u), t)
    merged, joined = g.group.stats()
    pipelined, faults = g.group.pipeline_stats()
    assert merged == STEPS - 1      # (step 0 is the first call of every sequence: single launches)
    assert joined == (merged if collide else 1), (merged, joined)      # only a round that starts a sequence joins
    assert pipelined == (merged if serve_max_wg else 0) and faults == 0, (pipelined, faults)      # the two-wave form runs with depth 1
    if collide:
        assert bool(touched)
    snaps = g.snapshots()
    for sn, n in zip(snaps, SIZES):
        assert int(sn["episodes"][0]) == int(sn["tally"][:, 0].sum()) >= 3 * n
    _finish(g, u)


@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_equals_ungrouped(depth):
    _run_pair(depth)


@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_equals_ungrouped_with_a_member_in_contact(depth):
    _run_pair(depth, collide=True)


@pytest.mark.parametrize("depth", [2, 3])
def test_the_two_wave_form_runs_with_depth_one(depth):
    """serve_wave_max_workgroups 0: two workgroups of the two-wave form fit one CU, so a waiting one could keep its predecessor off the chip - never pipelined"""
    _run_pair(depth, serve_max_wg=0)


@pytest.mark.parametrize("busy", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_warm_consumer(depth, busy):
    _run_pair(depth, warm=True, busy=busy)


def test_flush_mid_sequence_then_readers_on_a_member_stream_then_on():
    """Rounds are in flight behind a busy first launch stream; flush() ends the sequence, and clones queued on member 3's stream right after it - no host
    synchronisation - see the last round.  The next round starts a new sequence behind those clones."""
    g, u = _pipe_group(3), base.Set(False)
    clones = []
    for s in (g, u):
        for t in range(4):
            s.step(t)
        torch.cuda.synchronize()
        with torch.cuda.stream(s.members[0].stream):
            torch.cuda._sleep(10_000_000)
        for t in range(4, 7):
            s.step(t)
        if s.group is not None:
            s.group.flush()
        m = s.members[3]
        with torch.cuda.stream(m.stream):
            clones.append((m.env.flags[:m.n].clone(), m.env.step_count[:m.n].clone(), m.env.obs.clone(), m.env.last_reset.clone()))
        for t in range(7, 11):
            s.step(t)
    assert g.group.stats() == (10, 2) and g.group.pipeline_stats() == (10, 0)      # two sequences: the first round and the one after the flush joined
    torch.cuda.synchronize()
    for a, b in zip(*clones):
        assert torch.equal(a, b)
    _finish(g, u)


def test_option_switch_mid_sequence():
    g, u = _pipe_group(3), base.Set(False)
    t = 0
    for depth, n_pipe in ((None, 4), (1, 4), (2, 8), (3, 12)):
        if depth is not None:
            g.group.set_option("pipeline_depth", depth)
        for _ in range(5 if t == 0 else 4):
            g.step(t); u.step(t)
            t += 1
        base._equal(_device_snapshots(g), _device_snapshots(u), ("depth", depth))
        assert g.group.pipeline_stats() == (n_pipe, 0), (depth, g.group.pipeline_stats())
    assert g.group.stats()[0] == t - 1
    _finish(g, u)


def test_a_member_leaves_mid_sequence():
    g, u = _pipe_group(3), base.Set(False)
    for t in range(5):
        g.step(t); u.step(t)
    for s in (g, u):
        s.close_member(1)      # a launch stream of the running sequence goes with it: the next round starts a new one on the streams of members 0, 2 and 3
    for t in range(5, 11):
        g.step(t); u.step(t)
    base._equal(_device_snapshots(g), _device_snapshots(u), "three members")
    assert g.group.pipeline_stats() == (10, 0)
    for s in (g, u):
        s.close_member(0)
        s.close_member(2)      # one member, one stream: nothing to overlap with
    for t in range(11, 14):
        g.step(t); u.step(t)
    assert g.group.pipeline_stats() == (10, 0) and g.group.stats()[0] == 13
    _finish(g, u)


def test_option_values():
    from d3il_amd import capi
    g = base.Set(True)
    with pytest.raises(capi.D3ilError, match="error -1: pipeline_depth"):      # D3IL_EINVAL: not without quiet_streams
        g.group.set_option("pipeline_depth", 2)
    g.group.set_option("quiet_streams", 1)
    for bad in (0, 5):
        with pytest.raises(capi.D3ilError, match="error -1: pipeline_depth"):
            g.group.set_option("pipeline_depth", bad)
    g.group.set_option("dispatch_sets", 2)
    with pytest.raises(capi.D3ilError, match="error -1: pipeline_depth"):      # not with two dispatch sets
        g.group.set_option("pipeline_depth", 2)
    g.group.set_option("dispatch_sets", 1)
    g.group.set_option("pipeline_depth", 2)
    with pytest.raises(capi.D3ilError, match="error -1: dispatch_sets"):      # ... in either order
        g.group.set_option("dispatch_sets", 2)
    with pytest.raises(capi.D3ilError, match="error -1: quiet_streams"):
        g.group.set_option("quiet_streams", 0)
    for bad in (0, 600001):
        with pytest.raises(capi.D3ilError, match="error -1: pipeline_timeout_ms"):
            g.group.set_option("pipeline_timeout_ms", bad)
    g.group.set_option("pipeline_timeout_ms", 5000)
    for t in range(4):
        g.step(t)
    assert g.group.pipeline_stats() == (3, 0)
    g.members[0].snapshot()
    assert g.group.pipeline_stats() == (3, 0)
    g.close()


def test_depth_times_workgroups_above_the_cu_budget_runs_with_depth_one():
    """The group has four workgroups.  "pipeline_cu_budget" lowers the CU count the residency rule is checked against (it cannot raise it): with 7 CUs two
    rounds of four workgroups do not fit and the rounds run with depth 1, with 8 they are pipelined, and depth 3 needs 12."""
    from d3il_amd import capi
    g, u = _pipe_group(2), base.Set(False)
    for bad in (0, 1 << 20):
        with pytest.raises(capi.D3ilError, match="error -1: pipeline_cu_budget"):
            g.group.set_option("pipeline_cu_budget", bad)
    t, want = 0, 0
    for budget, depth, piped in ((7, 2, False), (8, 2, True), (11, 3, False), (12, 3, True)):
        g.group.set_option("pipeline_depth", depth)
        g.group.set_option("pipeline_cu_budget", budget)
        for _ in range(4):
            g.step(t); u.step(t)
            t += 1
        want += (3 if t == 4 else 4) if piped else 0
        assert g.group.pipeline_stats() == (want, 0), (budget, depth, g.group.pipeline_stats())
    assert g.group.stats()[0] == t - 1
    _finish(g, u)


def test_this_file_passes_on_the_poison_build():
    """-DD3IL_POISON: the LDS of the pipelined form starts as NaN like that of the other group forms (its own words are written before they are read)."""
    if os.environ.get("D3IL_LIB_PATH"):
        pytest.skip("already running on a variant library")
    if not os.path.exists(POISON):
        pytest.fail("libd3il_rollout_poison.so not built (python -c 'from d3il_amd import build; build.build_poison()')")
    env = dict(os.environ, D3IL_LIB_PATH=POISON)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "tests/test_gpu_avoiding_group_pipeline.py"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=3 * CHILD_S)
    print("poison child: %.1f s" % (time.perf_counter() - t0))
    assert r.returncode == 0, "\n".join(r.stdout.splitlines()[-15:])
