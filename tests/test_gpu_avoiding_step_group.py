"""The step group of the Avoiding rollout step (d3il_group_create).

The d3il_random_rollout_step calls that the members of a group make for one step go out as ONE dispatch: a call only marks its member pending, the call that
completes the round launches k_avoiding_step_split<true, SERVE, true>, whose workgroups find their member in a device table and then run the code of a launch
of that member alone.  Everything here compares a grouped set of handles bit for bit (np.array_equal) with the same handles ungrouped, every handle on a
stream of its own: state, flags, step counters, obs, done, success, mode, last_reset, actions, the harness pose, episode counts and tally.

Shapes: members of 64, 64, 40 and 1 environments - a whole workgroup, a second one (first workgroup index 1), a partial last workgroup (24 dead lanes) and one
live lane; four workgroups in the merged dispatch.  Episodes of 12 steps staggered over the lanes: every step times some lanes out, so tally, counters and the
reset epilogue run in every launch.  40 steps.  serve_wave_max_workgroups 256 / 0 on every member selects the three-wave / two-wave group form.

Poison build: the whole file passes in a child process on libd3il_rollout_poison.so (the group forms get the same LDS fills).  CHILD_S: the child's wall
time measured on one MI355X, process start included; its limit is three times that."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "oracle_avoiding_rollout.npz"))
POISON = os.path.join(ROOT, "d3il_amd", "libd3il_rollout_poison.so")
CHILD_S = 4.7
SEED = 31
SIZES = (64, 64, 40, 1)
MAX_STEPS, STEPS = 12, 40
COL = GOLD["collide__actions"]
COL_FROM = 78      # the golden `collide` rollout touches the obstacle after 82 steps: the driven member starts from its state after 78


class Member:
    def __init__(self, n, offset, serve_max_wg):
        from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
        self.n, self.offset = n, offset
        self.stream = torch.cuda.Stream(torch.device("cuda:0"))
        with torch.cuda.stream(self.stream):
            env = self.env = ObstacleAvoidanceVecEnv(n, device=0, max_steps_per_episode=MAX_STEPS)
            env.bind_stream(self.stream)
            env.set_option("serve_wave_max_workgroups", serve_max_wg)
            env.set_init_qpos(GOLD["init_qpos"])
            env.reset()
            env.step_count[:n] = (torch.arange(n, device=env.device, dtype=torch.int32) * 5 + offset) % MAX_STEPS
            env.policy_begin()
            self.table = env.set_tally(3, torch.arange(n, dtype=torch.int32) % 3)
            self.episodes = torch.zeros(2, dtype=torch.int64, device=env.device)
            self.actions = torch.zeros(n, 7, dtype=torch.float64, device=env.device)
            env.set_option("fuse_rollout_tail", 1)
        self.stream.synchronize()

    def call(self, t, override=None):
        """this member's d3il_random_rollout_step of step t; override: set-points written over the drawn action on the member's stream before the call"""
        if override is not None:
            with torch.cuda.stream(self.stream):
                self.actions.copy_(override)
        self.env.random_rollout_step(SEED, self.offset, t, self.actions, self.episodes)

    def device_snapshot(self):
        """device-side copies only (no library call: a library call on a member would end a round)"""
        env, n = self.env, self.n
        torch.cuda.synchronize()
        return {"state": env.state[:, :n].cpu().numpy(), "flags": env.flags[:n].cpu().numpy(), "step_count": env.step_count[:n].cpu().numpy(),
                "obs": env.obs.cpu().numpy(), "done": env.done.cpu().numpy(), "success": env.success.cpu().numpy(), "mode": env.mode.cpu().numpy(),
                "last_reset": env.last_reset.cpu().numpy(), "actions": self.actions.cpu().numpy(), "policy_des": env.policy_des[:, :n].cpu().numpy(),
                "tally": self.table.cpu().numpy(), "episodes": self.episodes.cpu().numpy()}

    def snapshot(self):
        snap = self.device_snapshot()
        st, fl, sc = self.env.get_state()      # through the API as well
        assert np.array_equal(st, snap["state"]) and np.array_equal(fl.view(np.int32), snap["flags"]) and np.array_equal(sc, snap["step_count"])
        return snap


class Set:
    def __init__(self, grouped, serve_max_wg=256):
        from d3il_amd.envs.avoiding import StepGroup
        off, self.members = 7000, []
        for n in SIZES:
            self.members.append(Member(n, off, serve_max_wg))
            off += n
        self.group = StepGroup([m.env for m in self.members]) if grouped else None

    def step(self, t, override=None):
        for i, m in enumerate(self.members):
            if m is not None:
                m.call(t, None if override is None else override(i, t))

    def snapshots(self):
        return [None if m is None else m.snapshot() for m in self.members]

    def close_member(self, i):
        self.members[i].env.close()
        self.members[i] = None

    def close(self):
        if self.group is not None:
            self.group.close()
        for m in self.members:
            if m is not None:
                m.env.close()


def _equal(sa, sb, where):
    assert len(sa) == len(sb)
    for i, (a, b) in enumerate(zip(sa, sb)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        for k in a:
            assert np.array_equal(a[k], b[k]), (where, "member", i, k, np.nonzero(np.atleast_1d(a[k] != b[k]))[-1][:8].tolist())


def _changed(before, after):
    """per member: did anything a step writes change"""
    return [any(not np.array_equal(b[k], a[k]) for k in ("state", "step_count", "actions")) for b, a in zip(before, after)]


_NEAR = {}


def _near_contact_column():
    """State column, flags and set-point of one environment after COL_FROM steps of the golden `collide` set-points (computed once per process)."""
    if not _NEAR:
        from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
        env = ObstacleAvoidanceVecEnv(64, device=0, max_steps_per_episode=250)
        env.set_init_qpos(GOLD["init_qpos"])
        env.reset()
        for t in range(COL_FROM):
            env.step(torch.as_tensor(np.repeat(COL[t][None], 64, 0), dtype=torch.float64, device=env.device))
        st, fl, sc = env.get_state()
        env.close()
        _NEAR.update(state=st[:, 0].copy(), flags=fl[0])
    return _NEAR


def _drive_member_to_contact(s, i):
    """member i of set s: every lane in the near-contact state at the start of a 12-step episode, the harness pose on the set-point it has reached"""
    from d3il_amd import capi
    near, m = _near_contact_column(), s.members[i]
    st = np.repeat(near["state"][:, None], m.n, axis=1)
    fl = np.full(m.n, near["flags"], dtype=np.uint32)
    assert not (fl & capi.FLAG_ROD_CONTACT).any() and not (fl & capi.FLAG_TERMINATED).any()      # not there yet
    m.env.set_state(st, fl, np.zeros(m.n, dtype=np.int32))
    with torch.cuda.stream(m.stream):
        m.env.policy_des[:, :m.n] = torch.as_tensor(COL[COL_FROM - 1][:3], dtype=torch.float64, device=m.env.device).unsqueeze(1)
    m.stream.synchronize()


def _run_pair(serve_max_wg, collide):
    from d3il_amd import capi
    g, u = Set(True, serve_max_wg), Set(False, serve_max_wg)
    override = None
    if collide:
        for s in (g, u):
            _drive_member_to_contact(s, 2)
        dev = torch.device("cuda:0")
        rows = [torch.as_tensor(np.repeat(COL[min(COL_FROM + t, len(COL) - 1)][None], SIZES[2], 0), dtype=torch.float64, device=dev) for t in range(STEPS)]
        # step 0 is the first call of a sequence: it draws inside the library call, behind anything the caller wrote
        override = lambda i, t: rows[t] if (i == 2 and t > 0) else None
    touched = torch.zeros((), dtype=torch.bool, device="cuda:0")
    retired_next = torch.zeros((), dtype=torch.bool, device="cuda:0")
    for t in range(STEPS):
        g.step(t, override); u.step(t, override)
        if collide:      # watched on the ungrouped set (no library call, no host synchronise): a touching lane, and a lane the following launch reset
            m = u.members[2]
            with torch.cuda.stream(m.stream):
                touched |= ((m.env.flags[:m.n] & capi.FLAG_ROD_CONTACT) != 0).any()
                retired_next |= touched & (m.env.last_reset != 0).any()
        if t in (0, 1, 13, STEPS - 1):
            _equal(g.snapshots(), u.snapshots(), t)      # (get_state on a group with nothing pending flushes nothing: the next round merges again)
    snaps = g.snapshots()
    for sn, n in zip(snaps, SIZES):
        assert int(sn["episodes"][0]) == int(sn["tally"][:, 0].sum()) >= 3 * n      # 40 steps of 12-step episodes
    if collide:
        assert bool(touched) and bool(retired_next)
    g.close(); u.close()


@pytest.mark.parametrize("serve_max_wg", [256, 0])
def test_grouped_equals_ungrouped(serve_max_wg):
    _run_pair(serve_max_wg, collide=False)


@pytest.mark.parametrize("serve_max_wg", [256, 0])
def test_grouped_equals_ungrouped_with_a_member_in_contact(serve_max_wg):
    """The 40-lane member on the golden `collide` set-points: its lanes ask the serving wave for the rod contact inside a merged launch, finish, and ride
    through the next merged launch retired before its epilogue resets them."""
    _run_pair(serve_max_wg, collide=True)


def test_nothing_moves_before_the_last_call_of_a_round():
    g = Set(True)
    g.step(0)      # first calls of the sequences: not merged
    for t in (1, 2, 3):
        before = [m.device_snapshot() for m in g.members]
        for m in g.members[:-1]:
            m.call(t)
        mid = [m.device_snapshot() for m in g.members]      # (device_snapshot synchronises the device)
        _equal(before, mid, t)
        g.members[-1].call(t)
        after = [m.device_snapshot() for m in g.members]
        assert all(_changed(before, after)), (t, _changed(before, after))
    g.close()


def test_partial_rounds_and_different_t():
    g, u = Set(True), Set(False)
    for t in range(3):
        g.step(t); u.step(t)
    # a partial round, then get_state on a pending member: members 0 and 1 run through the single path
    for s in (g, u):
        s.members[0].call(3); s.members[1].call(3)
    a, b = g.members[1].env.get_state(), u.members[1].env.get_state()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _equal([g.members[0].device_snapshot(), g.members[1].device_snapshot()], [u.members[0].device_snapshot(), u.members[1].device_snapshot()], "partial")
    # ... and d3il_step on a pending member
    for s in (g, u):
        s.members[2].call(3)
        s.members[2].env.step(s.members[2].actions)
        s.members[3].call(3)
    _equal(g.snapshots(), u.snapshots(), "step")
    # member 2's sequence was interrupted by d3il_step: its next call draws again and is not merged; the full round after it merges again
    g.step(4); u.step(4)
    _equal(g.snapshots(), u.snapshots(), 4)
    before = [m.device_snapshot() for m in g.members]
    for m in g.members[:-1]:
        m.call(5)
    _equal(before, [m.device_snapshot() for m in g.members], "merged again")
    g.members[-1].call(5)
    assert all(_changed(before, [m.device_snapshot() for m in g.members]))
    u.step(5)
    _equal(g.snapshots(), u.snapshots(), 5)
    # different t per member: every sequence jumps (first call, unmerged), then continues with its own t - eligible calls that fit no common round
    for k in range(3):
        for s in (g, u):
            for i, m in enumerate(s.members):
                m.call(100 * (i + 1) + k)
    _equal(g.snapshots(), u.snapshots(), "different t")
    g.close(); u.close()


def test_stream_order_is_kept_for_the_caller():
    """Member 1's stream is kept busy, then a torch write to its step counters is queued on it; the first member's stream is busy too.  The merged launch must
    see the write, and a clone of obs queued on a member's stream right after the round must see the launch.  No host synchronisation in between."""
    g, u = Set(True), Set(False)
    clones = []
    for s in (g, u):
        s.step(0); s.step(1)
        torch.cuda.synchronize()
        m1 = s.members[1]
        with torch.cuda.stream(s.members[0].stream):
            torch.cuda._sleep(10_000_000)
        with torch.cuda.stream(m1.stream):
            torch.cuda._sleep(20_000_000)
            m1.env.step_count[:m1.n] = MAX_STEPS - 1      # every lane of member 1 times out in the next step
        s.step(2)
        got = []
        for m in (s.members[1], s.members[3]):
            with torch.cuda.stream(m.stream):
                got.append((m.env.obs.clone(), m.env.last_reset.clone(), m.env.step_count[:m.n].clone()))
        clones.append(got)
    torch.cuda.synchronize()
    for (ga, gb, gc), (ua, ub, uc) in zip(*clones):
        assert torch.equal(ga, ua) and torch.equal(gb, ub) and torch.equal(gc, uc)
    assert bool(clones[0][0][1].all())      # the write was seen: all of member 1 was reset by that step
    _equal(g.snapshots(), u.snapshots(), "stream order")
    g.close(); u.close()


def test_timing_counts_the_merged_launch_once_per_member():
    g = Set(True)
    g.step(0)
    for m in g.members:
        m.env.set_timing(True)
    rounds = 6
    for t in range(1, 1 + rounds):
        g.step(t)
    last = [m.env.last_step_ms() for m in g.members]
    stats = [m.env.timing_stats() for m in g.members]
    assert all(s[3] == rounds for s in stats), stats
    assert all(s == stats[0] for s in stats) and 0.0 < stats[0][1] <= stats[0][2] <= stats[0][0], stats
    assert all(x == last[0] for x in last) and last[0] > 0.0, last
    for m in g.members:
        m.env.set_timing(False)
    g.close()


def test_timing_survives_the_end_of_the_group():
    """Timing stays on across the group's destruction.  The shared event pairs die with the group, so a member must not name them afterwards: the durations
    of the merged rounds are read when the member leaves (timing_stats keeps them), last_step_ms has no launch to report until the member's next timed launch,
    which is a single one with the member's own pair."""
    from d3il_amd import capi
    g = Set(True)
    g.step(0)
    for m in g.members:
        m.env.set_timing(True)
    rounds = 5
    for t in range(1, 1 + rounds):
        g.step(t)
    g.group.close(); g.group = None
    for m in g.members:
        with pytest.raises(capi.D3ilError, match="no step recorded"):
            m.env.last_step_ms()
    stats = [m.env.timing_stats() for m in g.members]
    assert all(s[3] == rounds for s in stats), stats
    assert all(s == stats[0] for s in stats) and 0.0 < stats[0][1] <= stats[0][2] <= stats[0][0], stats
    g.step(1 + rounds)      # ungrouped: every member launches on its own, with its own event pair
    assert all(m.env.last_step_ms() > 0.0 for m in g.members)
    after = [m.env.timing_stats() for m in g.members]
    assert all(a[3] == rounds + 1 and a[0] > s[0] for a, s in zip(after, stats)), (stats, after)
    # a member that is destroyed while the group lives on leaves in the same way; the group goes on timing the others
    h = Set(True)
    h.step(0)
    for m in h.members:
        m.env.set_timing(True)
    h.step(1); h.step(2)
    h.close_member(0)
    h.step(3)
    live = [m for m in h.members if m is not None]
    last = [m.env.last_step_ms() for m in live]
    assert all(x == last[0] for x in last) and last[0] > 0.0, last
    assert all(m.env.timing_stats()[3] == 3 for m in live)
    g.close(); h.close()


def test_destroying_a_member_and_the_group():
    g, u = Set(True), Set(False)
    for t in range(3):
        g.step(t); u.step(t)
    # mid-round: member 0 is pending when member 1 is destroyed
    for s in (g, u):
        s.members[0].call(3)
        s.close_member(1)
        for m in s.members[1:]:
            if m is not None:
                m.call(3)
    _equal(g.snapshots(), u.snapshots(), "after the destroy")
    for t in range(4, 8):
        g.step(t); u.step(t)
    _equal(g.snapshots(), u.snapshots(), 7)
    # three members still merge
    live = [m for m in g.members if m is not None]
    before = [m.device_snapshot() for m in live]
    for m in live[:-1]:
        m.call(8)
    _equal(before, [m.device_snapshot() for m in live], "three members")
    live[-1].call(8)
    u.step(8)
    _equal(g.snapshots(), u.snapshots(), 8)
    # without the group every call launches at once again
    g.group.close(); g.group = None
    before = live[0].device_snapshot()
    live[0].call(9)
    assert _changed([before], [live[0].device_snapshot()])[0]
    for m in live[1:]:
        m.call(9)
    u.step(9)
    for t in range(10, 13):
        g.step(t); u.step(t)
    _equal(g.snapshots(), u.snapshots(), 12)
    g.close(); u.close()


def test_this_file_passes_on_the_poison_build():
    """-DD3IL_POISON: the LDS of the group forms starts as NaN like that of the single forms."""
    if os.environ.get("D3IL_LIB_PATH"):
        pytest.skip("already running on a variant library")
    if not os.path.exists(POISON):
        pytest.fail("libd3il_rollout_poison.so not built (python -c 'from d3il_amd import build; build.build_poison()')")
    env = dict(os.environ, D3IL_LIB_PATH=POISON)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "tests/test_gpu_avoiding_step_group.py"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=3 * CHILD_S)
    assert r.returncode == 0, "\n".join(r.stdout.splitlines()[-15:])
