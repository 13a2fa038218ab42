"""Retired lanes of the Avoiding split step kernels.

A lane that is finished and not successful at step_begin (rod contact in the previous step, timeout, already terminated) is reset later in the same library
call - by the rollout epilogue of the fused step, or by the reset kernels of d3il_step_auto_reset - and nothing its 35 sub-steps compute survives that
reset.  The split kernels therefore keep such a lane out of the rare constraint paths (three-wave form: it asks the serving wave for nothing; two-wave form:
it does not enter rare_constraints).  Nothing observable may change: every test here drives one handle through the path that retires lanes and a second one
through the separate public calls (policy_action, step, auto_reset), which retire nothing, and compares state, flags, step counters, obs, done, success,
mode, last_reset, the harness pose, tally and episode counters with np.array_equal after every step.

Lane classes (i % 3): 0 follows the golden `collide` set-points (rod contact after 82 steps), 1 the golden `succeed` set-points (goal line after 158 steps),
2 keeps the policy's random walk and times out through a staggered step counter.  Every wave then holds retired and unretired lanes in the same launch.
n = 100: one full workgroup plus 36 live and 28 dead lanes; environment 99 collides, so the dead lanes (copies of environment n - 1) retire with it.
serve_wave_max_workgroups 256 / 0 selects k_avoiding_step_split<true, true> (three waves) / <true, false> (two waves).

Poison build: the whole file passes in a child process on libd3il_rollout_poison.so.  Measured on one MI355X, process start included: the child takes
6.3 s (CHILD_S); its limit is three times that."""
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
CHILD_S = 6.3
SEED, OFF = 23, 9000
MAX_STEPS = 250
COL, SUC = GOLD["collide__actions"], GOLD["succeed__actions"]


class Handle:
    """mode: 'fused' (random_rollout_step with fuse_rollout_tail: the epilogue retires), 'auto' (policy_action + step_auto_reset: the signalled step kernel
    retires), 'separate' (policy_action + step + auto_reset: the unretired reference)."""

    def __init__(self, n, serve_max_wg, mode, step_count=None):
        from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
        self.n, self.mode = n, mode
        env = self.env = ObstacleAvoidanceVecEnv(n, device=0, max_steps_per_episode=MAX_STEPS)
        env.set_option("serve_wave_max_workgroups", serve_max_wg)
        env.set_init_qpos(GOLD["init_qpos"])
        env.reset()
        if step_count is not None:
            env.step_count[:n] = torch.as_tensor(step_count, dtype=torch.int32, device=env.device)
        env.policy_begin()
        self.table = env.set_tally(3, torch.arange(n, dtype=torch.int32) % 3)
        self.episodes = torch.zeros(2, dtype=torch.int64, device=env.device)
        self.actions = torch.zeros(n, 7, dtype=torch.float64, device=env.device)
        if mode == "fused":
            env.set_option("fuse_rollout_tail", 1)
        self.finished = 0           # finished lanes counted on the host (separate: from done before the reset; the others: from last_reset)
        self.kinds = np.zeros(3, dtype=np.int64)      # separate handle only: contact, success and timeout endings seen before the reset cleared them
        self.ahead = self.drawn = None

    def _pair(self):
        return self.actions.cpu().numpy().copy(), self.env.policy_des[:, :self.n].cpu().numpy().copy()

    def forget_sequence(self):
        self.ahead = None

    def step(self, t, override=None):
        """override = (lane index tensor, rows): set-points written over the policy's draw for those lanes before the step kernel reads them"""
        from d3il_amd import capi
        env = self.env
        if self.mode == "fused":
            if override is not None:
                self.actions[override[0]] = override[1]
            env.random_rollout_step(SEED, OFF, t, self.actions, self.episodes)
            torch.cuda.synchronize()
            self.finished += int(env.last_reset.sum())
            self.ahead = self._pair()
            return
        env.policy_action(SEED, OFF, t, self.actions)
        self.drawn = self._pair()
        if override is not None:
            self.actions[override[0]] = override[1]
        if self.mode == "auto":
            env.step_auto_reset(self.actions, self.episodes)
            torch.cuda.synchronize()
            self.finished += int(env.last_reset.sum())
            return
        env.step(self.actions)
        torch.cuda.synchronize()
        done = env.done.cpu().numpy().astype(bool)
        ok = env.success.cpu().numpy() != 0
        fl = env.flags[:self.n].cpu().numpy()
        term = (fl & capi.FLAG_TERMINATED) != 0      # set at step_begin: by the goal line (with success) or by the rod contact the previous step left
        self.kinds += [int((done & ~ok & term).sum()), int((done & ok).sum()), int((done & ~term).sum())]
        self.finished += int(done.sum())
        env.auto_reset(self.episodes)
        torch.cuda.synchronize()

    def snapshot(self):
        env, n = self.env, self.n
        st, fl, sc = env.get_state()
        snap = {"state": st, "flags": fl, "step_count": sc, "obs": env.obs.cpu().numpy(), "done": env.done.cpu().numpy(), "success": env.success.cpu().numpy(),
                "mode": env.mode.cpu().numpy(), "last_reset": env.last_reset.cpu().numpy(), "tally": self.table.cpu().numpy(), "episodes": self.episodes.cpu().numpy()}
        # the fused handle has drawn the next step already: its x / y pose rows run one step ahead and are compared through the draw-ahead pair
        pd = env.policy_des[:, :n].cpu().numpy()
        snap["policy_des"] = pd[2:] if self.mode == "fused" else pd
        return snap

    def close(self):
        self.env.close()


def _same(a, b, where):
    sa, sb = a.snapshot(), b.snapshot()
    if a.mode == "fused":
        sb["policy_des"] = sb["policy_des"][2:]
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), (where, k, np.nonzero(np.atleast_1d(sa[k] != sb[k]))[-1][:8].tolist())
    return sa


def _step_both(a, b, t, override):
    """step t on the retiring handle a and the separate handle b, everything compared afterwards"""
    ahead = a.ahead
    a.step(t, override); b.step(t, override)
    if ahead is not None:      # what the fused handle drew ahead for this step == what the separate handle's policy_action has just drawn
        assert np.array_equal(ahead[0], b.drawn[0]), (t, "actions")
        assert np.array_equal(ahead[1], b.drawn[1]), (t, "policy_des")
    return _same(a, b, t)


def _totals(a, b, snap):
    assert a.finished == b.finished == int(snap["episodes"][0]) == int(snap["tally"][:, 0].sum()), (a.finished, b.finished, snap["episodes"], snap["tally"][:, 0])
    assert int(snap["episodes"][1]) == int(snap["tally"][:, 1].sum()) == int(snap["tally"][:, 2:].sum())
    assert int(snap["episodes"][1]) == int(b.kinds[1])


def _classes(n, dev):
    lanes = np.arange(n)
    col_i, suc_i = lanes[lanes % 3 == 0], lanes[lanes % 3 == 1]
    idx = torch.as_tensor(np.concatenate([col_i, suc_i]), device=dev)
    # class 2 times out between steps 3 and 3 + 39 of the run, a few lanes per step, and not again within it
    sc = np.where(lanes % 3 == 2, MAX_STEPS - 4 - (lanes // 3) % 40, 0)

    def override(t):
        # step 0 keeps the policy's own draw (the first call of a fused sequence draws inside the library call, behind anything the caller wrote)
        if t == 0:
            return None
        rows = np.concatenate([np.repeat(COL[min(t - 1, len(COL) - 1)][None], len(col_i), 0), np.repeat(SUC[min(t - 1, len(SUC) - 1)][None], len(suc_i), 0)])
        return idx, torch.as_tensor(rows, dtype=torch.float64, device=dev)
    return sc, override


def _mixed(n, serve_max_wg, mode):
    dev = torch.device("cuda:0")
    sc, override = _classes(n, dev)
    a, b = Handle(n, serve_max_wg, mode, sc), Handle(n, serve_max_wg, "separate", sc)
    for t in range(len(SUC) + 12):
        snap = _step_both(a, b, t, override(t))
    contact, success, timeout = b.kinds
    assert contact >= (n + 2) // 3 and success >= (n + 1) // 3 and timeout >= n // 3, b.kinds
    _totals(a, b, snap)
    a.close(); b.close()


@pytest.mark.parametrize("n,serve_max_wg", [(100, 256), (100, 0), (128, 256), (128, 0)])
def test_mixed_waves_fused_step_equals_the_separate_calls(n, serve_max_wg):
    assert (n - 1) % 3 == 0 or n == 128      # n = 100: environment n - 1 collides, the dead lanes of its wave copy it
    _mixed(n, serve_max_wg, "fused")


@pytest.mark.parametrize("serve_max_wg", [256, 0])
def test_step_auto_reset_equals_step_then_auto_reset(serve_max_wg):
    """d3il_step_auto_reset tells the split step kernel that its reset kernels follow in the same library call; the public step and auto_reset called
    separately retire nothing.  Same overridden set-points, contact, success and timeout endings."""
    _mixed(100, serve_max_wg, "auto")


@pytest.mark.parametrize("serve_max_wg", [256, 0])
def test_a_workgroup_whose_lanes_all_retire(serve_max_wg):
    """64 + 64 environments on the same collide set-points: every lane of both physics waves touches the obstacle in the same step and retires in the next
    launch - no lane asks the serving wave, which still sees one post per sub-step; the launch ends and the bits are equal."""
    n = 128
    dev = torch.device("cuda:0")
    idx = torch.arange(n, device=dev)
    a, b = Handle(n, serve_max_wg, "fused"), Handle(n, serve_max_wg, "separate")
    all_at_once = False
    for t in range(len(COL) + 8):
        ov = None if t == 0 else (idx, torch.as_tensor(np.repeat(COL[min(t - 1, len(COL) - 1)][None], n, 0), dtype=torch.float64, device=dev))
        before = b.kinds[0]
        snap = _step_both(a, b, t, ov)
        all_at_once = all_at_once or (b.kinds[0] - before >= 64 and bool(snap["last_reset"][:64].all() or snap["last_reset"][64:].all()))
    assert all_at_once, b.kinds
    _totals(a, b, snap)
    a.close(); b.close()


@pytest.mark.parametrize("serve_max_wg", [256, 0])
def test_interruption_while_lanes_are_about_to_retire(serve_max_wg):
    """After the step in which the rods first touch, every lane is about to retire.  Then, between two fused steps, set_state takes the contact flag away
    from two thirds of the lanes - one third is unfinished at the next step_begin and must get its contact solves, rod still pressed against the obstacle;
    the other is moved to the last step of its episode and retires by timeout instead - and a masked reset takes a fifth of the lanes out altogether.  The
    kernel has to decide from the state it loads.  (The step after an interruption is the first call of a new fused sequence and draws its own action: no
    override there, on either handle.)"""
    from d3il_amd import capi
    n = 100
    dev = torch.device("cuda:0")
    idx = torch.arange(n, device=dev)
    lanes = np.arange(n)
    a, b = Handle(n, serve_max_wg, "fused"), Handle(n, serve_max_wg, "separate")
    interrupted_at = None
    for t in range(len(COL) + 12):
        first_of_sequence = t == 0 or interrupted_at == t - 1
        ov = None if first_of_sequence else (idx, torch.as_tensor(np.repeat(COL[min(t - 1, len(COL) - 1)][None], n, 0), dtype=torch.float64, device=dev))
        before = b.kinds.copy()
        snap = _step_both(a, b, t, ov)
        if interrupted_at == t - 1:
            assert (b.kinds - before).tolist() == expected, (b.kinds - before, expected)
        touching = (snap["flags"] & capi.FLAG_ROD_CONTACT) != 0
        if interrupted_at is None and touching.any():
            interrupted_at = t
            kept = lanes % 5 != 2
            # what the next step must end: the lanes that keep their contact flag, by contact; the lanes moved to their last step, by timeout
            expected = [int((kept & (lanes % 3 == 2) & touching).sum()), 0, int((kept & (lanes % 3 == 1)).sum())]
            assert expected[0] > 0 and int((kept & (lanes % 3 == 0) & touching).sum()) > 0, touching.sum()
            st, fl, sc = b.env.get_state()
            fl = np.where(lanes % 3 != 2, fl & ~np.uint32(capi.FLAG_ROD_CONTACT), fl).astype(np.uint32)
            sc = np.where(lanes % 3 == 1, MAX_STEPS - 1, sc).astype(np.int32)
            a.env.set_state(st, fl, sc); b.env.set_state(st, fl, sc)
            m = (torch.arange(n, device=dev) % 5 == 2).to(torch.uint8)
            a.env.reset(m.clone()); b.env.reset(m.clone())
            a.forget_sequence()
            torch.cuda.synchronize()
            assert np.array_equal(a.env.policy_des[:, :n].cpu().numpy(), b.env.policy_des[:, :n].cpu().numpy())
    assert interrupted_at is not None and interrupted_at < len(COL) + 8
    _totals(a, b, snap)
    a.close(); b.close()


def test_this_file_passes_on_the_poison_build():
    """-DD3IL_POISON: the exchange area of the serving wave starts as NaN and a retired lane puts nothing into it."""
    if os.environ.get("D3IL_LIB_PATH"):
        pytest.skip("already running on a variant library")
    if not os.path.exists(POISON):
        pytest.fail("libd3il_rollout_poison.so not built (python -c 'from d3il_amd import build; build.build_poison()')")
    env = dict(os.environ, D3IL_LIB_PATH=POISON)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "tests/test_gpu_avoiding_retired_lanes.py"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=3 * CHILD_S)
    assert r.returncode == 0, "\n".join(r.stdout.splitlines()[-15:])
