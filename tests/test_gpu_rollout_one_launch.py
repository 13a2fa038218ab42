"""One launch per rollout step (option fuse_rollout_tail on the Avoiding split step kernels) and the cached reset image.

With the option on, a continuing d3il_random_rollout_step launches the step kernel only: its physics wave does, as an epilogue for its own lane, what the
harness does between two steps (finished mask, episode counters and tally, reset of a finished lane from the handle's cached post-reset image, re-latch of
the harness pose, the NEXT step's Philox action).  Everything here compares that handle bit for bit (np.array_equal) with a second handle driven through the
separate calls policy_action, step, auto_reset - which themselves copy the cached image - and the cached image with an explicit reset().

`actions` and the x / y rows of `policy_des` run one step ahead on the fused handle (the epilogue has drawn step t + 1 already), so they are compared with
what the separate handle holds right after ITS policy_action of step t + 1.

Shapes: 192 environments = three full workgroups; 100 = 28 dead lanes in the last workgroup (they must count nothing and draw nothing: the tally and episode
totals are compared with the finished lanes counted on the host: the separate handle counts them from `done` between its step and its auto_reset, the fused
handle - whose `done` is cleared again inside the launch - from `last_reset`, which the code under test writes; the two counts are compared with each other
and with the device's totals).  serve_wave_max_workgroups 256 / 0 selects k_avoiding_step_split<true, true> (three
waves) / <true, false> (two waves).  Episodes of 6 steps staggered i % 6: every step resets some lanes.

Poison build: the whole file passes in a child process on libd3il_rollout_poison.so.  Measured on one MI355X, process start included: the child takes up to
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
SEED, OFF = 11, 5000


class Handle:
    def __init__(self, n, serve_max_wg, fused, max_steps=6, init_qpos=None, stagger=True):
        from d3il_amd.envs.avoiding import ObstacleAvoidanceVecEnv
        self.n, self.fused = n, fused
        env = self.env = ObstacleAvoidanceVecEnv(n, device=0, max_steps_per_episode=max_steps)
        env.set_option("serve_wave_max_workgroups", serve_max_wg)
        env.set_init_qpos(GOLD["init_qpos"] if init_qpos is None else init_qpos)
        env.reset()
        if stagger:
            env.step_count[:n] = torch.arange(n, device=env.device, dtype=torch.int32) % max_steps
        env.policy_begin()
        self.table = env.set_tally(3, torch.arange(n, dtype=torch.int32) % 3)
        self.episodes = torch.zeros(2, dtype=torch.int64, device=env.device)
        self.actions = torch.zeros(n, 7, dtype=torch.float64, device=env.device)
        if fused:
            env.set_option("fuse_rollout_tail", 1)
        self.finished = 0           # finished lanes, counted on the host (fused: from last_reset; separate: from done)
        self.ahead = None           # (actions, policy_des) the fused handle holds for the NEXT step
        self.drawn = None           # the same pair of the separate handle right after its policy_action

    def _pair(self):
        return self.actions.cpu().numpy().copy(), self.env.policy_des[:, :self.n].cpu().numpy().copy()

    def step(self, t, override=None):
        """One rollout step.  override: actions written over the policy's draw before the step kernel reads them (both handles alike)."""
        env = self.env
        if self.fused:
            if override is not None:
                self.actions.copy_(override)
            env.random_rollout_step(SEED, OFF, t, self.actions, self.episodes)
            torch.cuda.synchronize()
            self.finished += int(env.last_reset.sum())
            self.ahead = self._pair()
        else:
            env.policy_action(SEED, OFF, t, self.actions)
            self.drawn = self._pair()
            if override is not None:
                self.actions.copy_(override)
            env.step(self.actions)
            self.finished += int(env.done.sum())
            env.auto_reset(self.episodes)
            torch.cuda.synchronize()

    def snapshot(self):
        env, n = self.env, self.n
        st, fl, sc = env.get_state()
        return {"state": st, "flags": fl, "step_count": sc, "obs": env.obs.cpu().numpy(), "done": env.done.cpu().numpy(), "success": env.success.cpu().numpy(),
                "mode": env.mode.cpu().numpy(), "last_reset": env.last_reset.cpu().numpy(), "policy_des_z": env.policy_des[2, :n].cpu().numpy(),
                "tally": self.table.cpu().numpy(), "episodes": self.episodes.cpu().numpy()}

    def close(self):
        self.env.close()


def _same(a, b, where):
    sa, sb = a.snapshot(), b.snapshot()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), (where, k, np.nonzero(np.atleast_1d(sa[k] != sb[k]))[0][:8].tolist())
    return sa


def _same_draw(fused_ahead, sep_drawn, where):
    """what the fused handle drew ahead for this step == what the separate handle's policy_action has just drawn"""
    assert fused_ahead is not None and sep_drawn is not None
    assert np.array_equal(fused_ahead[0], sep_drawn[0]), (where, "actions")
    assert np.array_equal(fused_ahead[1], sep_drawn[1]), (where, "policy_des")


def _run(a, b, t0, steps, override=None):
    """steps t0 .. t0 + steps - 1 on the fused handle a and the separate handle b, compared after every step"""
    for t in range(t0, t0 + steps):
        ahead = a.ahead
        ov = None if override is None else override(t)
        a.step(t, ov); b.step(t, ov)
        if ahead is not None:
            _same_draw(ahead, b.drawn, t)
        snap = _same(a, b, t)
    return snap


def _totals(a, b, snap):
    assert a.finished == b.finished == int(snap["episodes"][0]) == int(snap["tally"][:, 0].sum()), (a.finished, b.finished, snap["episodes"], snap["tally"][:, 0])
    assert int(snap["episodes"][1]) == int(snap["tally"][:, 1].sum()) == int(snap["tally"][:, 2:].sum())


@pytest.mark.parametrize("n,serve_max_wg", [(192, 256), (192, 0), (100, 256), (100, 0)])
def test_fused_step_equals_the_separate_calls(n, serve_max_wg):
    a, b = Handle(n, serve_max_wg, True), Handle(n, serve_max_wg, False)
    snap = _run(a, b, 0, 30)
    _totals(a, b, snap)
    assert a.finished >= 4 * n          # 30 steps of 6-step episodes: every lane finished at least four times
    # the last draw ahead: the separate handle's next policy_action gives it
    b.env.policy_action(SEED, OFF, 30, b.actions)
    _same_draw(a.ahead, b._pair(), "final")
    a.close(); b.close()


def test_rod_contact_and_success_pass_through_the_epilogue():
    """The set-points of the golden `collide` (rod contact after 82 steps) and `succeed` (goal line after 158 steps) rollouts, written over the policy's draw:
    the first half of the lanes collides, the second succeeds; both kinds finish inside the fused kernel and are counted, reset and re-latched there.  Step 0
    keeps the policy's own draw (the first call of a sequence draws inside the library call, behind anything the caller wrote): the absolute set-points
    follow one step late, and the test asserts that both kinds of ending were reached before it compares totals."""
    from d3il_amd import capi
    n = 128
    col, suc = GOLD["collide__actions"], GOLD["succeed__actions"]
    T = len(suc) + 12
    dev = torch.device("cuda:0")

    def override(t):
        rows = np.empty((n, 7))
        rows[:n // 2] = col[min(t - 1, len(col) - 1)]
        rows[n // 2:] = suc[min(t - 1, len(suc) - 1)]
        return torch.as_tensor(rows, dtype=torch.float64, device=dev)

    a, b = Handle(n, 256, True, max_steps=250, stagger=False), Handle(n, 256, False, max_steps=250, stagger=False)
    contact = success = 0
    for t in range(T):
        ahead = a.ahead
        ov = override(t) if t else None
        a.step(t, ov)
        # the separate handle, with a look at what finished before its auto-reset clears it
        b.env.policy_action(SEED, OFF, t, b.actions)
        b.drawn = b._pair()
        if ov is not None:
            b.actions.copy_(ov)
        b.env.step(b.actions)
        torch.cuda.synchronize()
        done = b.env.done.cpu().numpy().astype(bool)
        fl = b.env.flags[:n].cpu().numpy()
        contact += int((done & ((fl & capi.FLAG_ROD_CONTACT) != 0)).sum())
        success += int((done & (b.env.success.cpu().numpy() != 0)).sum())
        b.finished += int(done.sum())
        b.env.auto_reset(b.episodes)
        torch.cuda.synchronize()
        if ahead is not None:
            _same_draw(ahead, b.drawn, t)
        snap = _same(a, b, t)
    assert contact >= n // 2 and success >= n // 2, (contact, success)
    _totals(a, b, snap)
    assert int(snap["episodes"][1]) == success
    a.close(); b.close()


def test_interrupted_sequences():
    """policy_begin, a masked reset and set_state between fused steps end the prepared action (the harness pose goes back to where the draw started); the same
    calls on the separate handle give the same bits afterwards."""
    n = 100
    a, b = Handle(n, 256, True), Handle(n, 256, False)
    dev = a.env.device
    _run(a, b, 0, 4)
    m = (torch.arange(n, device=dev) % 2 == 0).to(torch.uint8)
    a.env.policy_begin(m); b.env.policy_begin(m)
    a.ahead = None
    torch.cuda.synchronize()
    assert np.array_equal(a.env.policy_des[:, :n].cpu().numpy(), b.env.policy_des[:, :n].cpu().numpy())
    _run(a, b, 4, 3)
    m = (torch.arange(n, device=dev) % 3 == 1).to(torch.uint8)
    a.env.reset(m.clone()); b.env.reset(m.clone())
    a.ahead = None
    torch.cuda.synchronize()
    assert np.array_equal(a.env.policy_des[:, :n].cpu().numpy(), b.env.policy_des[:, :n].cpu().numpy())
    _run(a, b, 7, 3)
    st, fl, sc = b.env.get_state()
    sc = (sc + 2) % 6
    a.env.set_state(st, fl, sc); b.env.set_state(st, fl, sc)
    a.ahead = None
    torch.cuda.synchronize()
    assert np.array_equal(a.env.policy_des[:, :n].cpu().numpy(), b.env.policy_des[:, :n].cpu().numpy())
    snap = _run(a, b, 10, 4)
    # a jump of the caller's step counter does not continue the sequence either
    a.ahead = None
    snap = _run(a, b, 20, 3)
    assert int(snap["episodes"][0]) == a.finished == b.finished
    a.close(); b.close()


def test_cache_follows_init_qpos():
    """set_init_qpos with a second pose after some steps: lanes auto-reset afterwards get the image of an explicit reset() on a fresh handle with that pose,
    lanes reset earlier keep the first pose."""
    from d3il_amd import capi
    n = 100
    q1 = GOLD["init_qpos"].copy()
    q2 = q1 + np.array([0.0, 0.02, 0.0, -0.03, 0.0, 0.01, 0.0])
    img = []
    for q in (q1, q2):
        f = Handle(64, 256, False, init_qpos=q, stagger=False)
        torch.cuda.synchronize()
        st, fl, sc = f.env.get_state()
        img.append((st[:, 0].copy(), int(fl[0]), int(sc[0]), f.env.obs[0].cpu().numpy().copy()))
        f.close()
    assert not np.array_equal(img[0][0], img[1][0])
    a, b = Handle(n, 256, True, init_qpos=q1), Handle(n, 256, False, init_qpos=q1)
    seen = [np.zeros(n, bool), np.zeros(n, bool)]
    keep = None
    for t in range(6):
        if t == 3:
            before = a.env.get_state()
            a.env.set_init_qpos(q2); b.env.set_init_qpos(q2)
            after = a.env.get_state()
            assert all(np.array_equal(x, y) for x, y in zip(before, after))      # nothing already reset moves
            # the lanes reset by step 2, under the first pose, still hold its image now that the pose has changed
            assert keep is not None and keep.any()
            assert np.array_equal(after[0][:, keep], np.repeat(img[0][0][:, None], int(keep.sum()), axis=1))
        ahead = a.ahead
        a.step(t); b.step(t)
        if ahead is not None:
            _same_draw(ahead, b.drawn, t)
        snap = _same(a, b, t)
        which = 0 if t < 3 else 1
        r = snap["last_reset"].astype(bool)
        assert r.any()
        st_img, fl_img, sc_img, obs_img = img[which]
        assert np.array_equal(snap["state"][:, r], np.repeat(st_img[:, None], int(r.sum()), axis=1)), t
        assert (snap["flags"][r] == fl_img).all() and (snap["step_count"][r] == sc_img).all()
        assert np.array_equal(snap["obs"][r], np.repeat(obs_img[None], int(r.sum()), axis=0))
        assert (snap["policy_des_z"][r] == st_img[capi.STATE_TCP + 2]).all()      # re-latched to the TCP of that pose
        seen[which] |= r
        if t == 2:
            keep = r.copy()
    assert seen[0].any() and seen[1].any() and not (seen[0] & seen[1]).any()
    a.close(); b.close()


def test_one_wave_step_kernel_keeps_the_tail_kernel():
    """split_waves = 0: the one-wave step kernel has no epilogue; fuse_rollout_tail then runs k_avoiding_tail behind it - same bits."""
    n = 100
    a, b = Handle(n, 256, True), Handle(n, 256, False)
    a.env.set_option("split_waves", 0); b.env.set_option("split_waves", 0)
    snap = _run(a, b, 0, 8)
    _totals(a, b, snap)
    a.close(); b.close()


def test_this_file_passes_on_the_poison_build():
    """-DD3IL_POISON: every LDS word of the split kernel's workgroup starts as NaN; the epilogue's two arguments are parked in LDS by the launch itself."""
    if os.environ.get("D3IL_LIB_PATH"):
        pytest.skip("already running on a variant library")
    if not os.path.exists(POISON):
        pytest.fail("libd3il_rollout_poison.so not built (python -c 'from d3il_amd import build; build.build_poison()')")
    env = dict(os.environ, D3IL_LIB_PATH=POISON)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "tests/test_gpu_rollout_one_launch.py"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=3 * CHILD_S)
    assert r.returncode == 0, "\n".join(r.stdout.splitlines()[-15:])
