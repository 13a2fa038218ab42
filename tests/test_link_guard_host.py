"""Link-near guard, the kernel's math on the CPU (T3): the host build of csrc/link_guard.h (tests/hostcheck/link_guard_check.cpp) against the NumPy
reference of tests/link_guard_reference.py for seeded random arm and cube poses of the three generic-engine tasks.

Required: the guard is raised whenever the reference distance is < margin - 1 mm and is not raised whenever it is > margin + slack + 1 mm (slack =
LG_SLACK of link_guard.h: how far the kernel's lower bound may lie below the true distance; the 1 mm covers the reference's sampling of the segments).
Cases in the band between are left out.  The sampler (joint vectors around the task's initial pose, clipped to jnt_range; cubes near and under the hand) was
tuned with the reference ALONE until at least 20 % of the cases are raised, 20 % are not and at most 2 % fall into the band; then the seed was fixed."""
import os

import numpy as np
import pytest

from d3il_amd import capi
from d3il_amd.model import blob as blob_mod
from tests.hostcheck.link_guard_check import LinkGuardHost
from tests.link_guard_reference import GuardReference, point_box_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "ref_offline_ik.npz"))
KEY = {"pushing": "avoiding__traj_last", "sorting": "sorting__traj_last", "inserting": "avoiding__traj_last"}
SEED, CASES = 20261016, 500


def _setup(task):
    host = LinkGuardHost(blob_mod.load(task))
    ref = GuardReference(task, (host.st_c, host.st_h, host.st_R))
    host.set(ref.capsule_array(), ref.margin)
    assert host.slack == capi.LINK_GUARD_SLACK and np.array_equal(host.box_half, ref.box_half) and host.nb == ref.nb
    return host, ref


def _draw(ref, task, rng, n):
    q0 = np.concatenate([G[KEY[task]], [0.0, 0.0]])
    out = []
    for _ in range(n):
        s = rng.uniform(0.02, 0.6)
        q = q0 + rng.uniform(-s, s, 9)
        q[7:] = rng.uniform(0.0, 0.04, 2)
        q = np.clip(q, ref.jnt_range[:, 0], ref.jnt_range[:, 1])
        cubes = np.zeros((ref.nb, 7))
        cubes[:, 0] = rng.uniform(0.35, 0.7, ref.nb)
        cubes[:, 1] = rng.uniform(-0.45, -0.1, ref.nb)
        cubes[:, 2] = rng.uniform(0.0, 0.12, ref.nb) + (0.1 if task == "sorting" else 0.0)
        qq = rng.normal(size=(ref.nb, 4)) * np.array([1, 0.15, 0.15, 1])
        cubes[:, 3:] = qq / np.linalg.norm(qq, axis=1)[:, None]
        out.append((q, cubes))
    return out


@pytest.mark.parametrize("task", ["pushing", "sorting", "inserting"])
def test_host_verdict_equals_brute_force(task):
    host, ref = _setup(task)
    cases = _draw(ref, task, np.random.default_rng(SEED), CASES)
    d = np.array([ref.distance(q, c)[0] for q, c in cases])
    m, slack = ref.margin, host.slack
    must, must_not = d < m - 1e-3, d > m + slack + 1e-3
    print("%s: raised %.3f, not raised %.3f, band %.4f" % (task, must.mean(), must_not.mean(), 1 - must.mean() - must_not.mean()))
    # the reference alone: both outcomes occur, the band is thin
    assert must.mean() >= 0.2 and must_not.mean() >= 0.2 and 1 - must.mean() - must_not.mean() <= 0.02
    got = np.array([host.eval(q, c)[0] for q, c in cases])
    assert got[must].all(), "false negatives at reference distances %s" % d[must & ~got]
    assert not got[must_not].any(), "false positives at reference distances %s" % d[must_not & got]


def test_capsules_are_placed_where_the_reference_puts_them():
    """The kernel's forward kinematics (PandaConsts chain, welded bodies folded into their link, finger slides) against the body-tree walk of the reference."""
    for task in KEY:
        host, ref = _setup(task)
        worst = 0.0
        for q, cubes in _draw(ref, task, np.random.default_rng(SEED + 1), 40):
            wc = host.eval(q, cubes)[1]
            for i, (a, b, r, st) in enumerate(ref.capsules_world(q)):
                worst = max(worst, np.abs(wc[i, :3] - a).max(), np.abs(wc[i, 3:6] - b).max(), abs(wc[i, 6] - r))
        assert worst < 1e-12, (task, worst)


def test_segment_box_bound_is_a_lower_bound_within_the_slack():
    """The bisection's value against a 0.1 mm sampling of the segment: never above the sampled distance (lower bound; the sampled one is itself an upper
    bound of the true distance), never more than slack + the sampling error below it.  Segments up to LG_MAXLEN, boxes like the scene's, inside / outside / grazing."""
    host, _ = _setup("pushing")
    rng = np.random.default_rng(SEED + 2)
    for _ in range(300):
        h = rng.uniform(0.01, 0.3, 3)
        qq = rng.normal(size=4)
        from tests.link_guard_reference import quat2mat
        R = quat2mat(qq / np.linalg.norm(qq))
        c = rng.uniform(-0.3, 0.3, 3)
        a = c + rng.uniform(-0.6, 0.6, 3)
        u = rng.normal(size=3)
        b = a + u / np.linalg.norm(u) * rng.uniform(0.0, 1.0) * rng.choice([0.05, 0.3, 1.0])
        n = int(np.ceil(np.linalg.norm(b - a) / 1e-4)) + 1
        P = a + np.linspace(0, 1, n)[:, None] * (b - a)
        sampled = point_box_distance(P, c, R, h).min()
        lb = host.seg_box(a, b, c, R.reshape(9), h)
        assert lb <= sampled + 1e-12 and lb >= sampled - host.slack - 0.5e-4 - 1e-12, (lb, sampled)


def test_bad_arguments_are_refused():
    host, ref = _setup("pushing")
    caps = ref.capsule_array()
    names = [b["name"] for b in ref.bodies]
    for bad, what in ((dict(row=0, col=8, val=0.0), "r must be positive"), (dict(row=0, col=0, val=names.index("push_box")), "outside the robot's chain"),
                      (dict(row=0, col=0, val=names.index("table_plane")), "outside the robot's chain"), (dict(row=0, col=0, val=999), "outside the model"),
                      (dict(row=0, col=5, val=5.0), "longer than 1 m")):
        c = caps.copy()
        c[bad["row"], bad["col"]] = bad["val"]
        with pytest.raises(ValueError, match=what):
            host.set(c, 0.02)
    with pytest.raises(ValueError, match="margin"):
        host.set(caps, -0.01)
    with pytest.raises(ValueError, match="0 .. 16"):
        host.set(np.tile(caps, (2, 1)), 0.02)
    host.set(caps[:0], 0.02)      # n = 0: off
    assert host.eval(np.zeros(9), np.tile([0.5, 0, 0, 1, 0, 0, 0], (ref.nb, 1)))[0] is False
