"""NumPy reference of the link-near guard, written for the tests (no library code): forward kinematics from the blob JSON's body tree
(``pos`` / ``quat`` of every body, hinge and slide joints about / along their ``axis``), the committed capsules placed by it, every segment
sampled at <= 1 mm spacing, closed-form point <-> oriented-box distance, minimum minus ``r`` over the guard's pair set: every capsule x every
cube, the capsules marked ``statics`` x every static box.  The static boxes are the generic engine's own list (GenConsts::st_c / st_h / st_R,
read back from the host build); the cube half extents come from the blob's geoms."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPSULES = os.path.join(ROOT, "d3il_amd", "model", "blobs", "panda_link_capsules.json")
SPACING = 1e-3


def quat2mat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def axis_angle(axis, a):
    u = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def point_box_distance(P, c, R, h):
    """Distance of the points P [n, 3] (world) from the box with centre c, world <- box rotation R [3, 3] and half extents h."""
    X = (P - c) @ R
    return np.linalg.norm(np.maximum(np.abs(X) - h, 0.0), axis=1)


class GuardReference:
    def __init__(self, task, statics):
        """statics: (centres [ns, 3], half extents [ns, 3], rotations [ns, 3, 3]) of the engine's static boxes."""
        with open(os.path.join(ROOT, "d3il_amd", "model", "blobs", task + ".json")) as f:
            self.js = json.load(f)
        with open(CAPSULES) as f:
            cj = json.load(f)
        self.margin = float(cj["margin"])
        self.bodies = self.js["bodies"]
        names = [b["name"] for b in self.bodies]
        self.caps = [(names.index(c["body"]), bool(c["statics"]), np.array(c["p0"]), np.array(c["p1"]), float(c["r"])) for c in cj["capsules"]]
        self.qadr = {a["joint"]: i for i, a in enumerate(self.js["actuators"])}      # qpos rows 0 .. 8 in actuator order
        self.st_c, self.st_h, self.st_R = statics
        objs = self.js["task_const"]["objects"]
        self.nb = len(objs)
        g = next(g for g in self.js["geoms"] if g["body"] == names.index(objs[0]) and g["type"] == "box")
        self.box_half = np.array(g["size"][:3], dtype=np.float64)
        self.jnt_range = np.zeros((9, 2))
        for b in self.bodies:
            for j in b["joints"]:
                if j["name"] in self.qadr:
                    self.jnt_range[self.qadr[j["name"]]] = j["range"]

    def capsule_array(self):
        """[n, 9] as d3il_set_link_guard takes it."""
        return np.array([[b, float(s)] + list(p0) + list(p1) + [r] for b, s, p0, p1, r in self.caps])

    def fk(self, q):
        frames = [(np.eye(3), np.zeros(3))]
        for i, b in enumerate(self.bodies[1:], start=1):
            Rp, pp = frames[b["parent"]]
            R, p = Rp @ quat2mat(b["quat"]), pp + Rp @ np.asarray(b["pos"], dtype=np.float64)
            for j in b["joints"]:
                if j["name"] not in self.qadr:
                    continue
                a = q[self.qadr[j["name"]]]
                if j["type"] == "hinge":
                    assert not np.any(j["pos"])
                    R = R @ axis_angle(j["axis"], a)
                elif j["type"] == "slide":
                    p = p + R @ (np.asarray(j["axis"], dtype=np.float64) * a)
            frames.append((R, p))
        return frames

    def capsules_world(self, q):
        fr = self.fk(q)
        return [(fr[b][1] + fr[b][0] @ p0, fr[b][1] + fr[b][0] @ p1, r, s) for b, s, p0, p1, r in self.caps]

    def distance(self, q, cubes):
        """(smallest capsule <-> box distance over the pair set, (capsule index, 'cube' / 'static', box index)).  cubes [nb, 7] = pos, quat."""
        cubes = np.asarray(cubes, dtype=np.float64).reshape(self.nb, 7)
        best, who = np.inf, None
        cube_R = [quat2mat(c[3:7]) for c in cubes]
        for ci, (a, b, r, st) in enumerate(self.capsules_world(q)):
            n = int(np.ceil(np.linalg.norm(b - a) / SPACING)) + 1
            P = a + np.linspace(0.0, 1.0, n)[:, None] * (b - a)
            for k in range(self.nb):
                d = point_box_distance(P, cubes[k, :3], cube_R[k], self.box_half).min() - r
                if d < best:
                    best, who = d, (ci, "cube", k)
            if st:
                for s in range(len(self.st_c)):
                    d = point_box_distance(P, self.st_c[s], self.st_R[s], self.st_h[s]).min() - r
                    if d < best:
                        best, who = d, (ci, "static", s)
        return best, who

    def cube_distance(self, q, cubes):
        """Smallest distance over the capsule <-> cube pairs only."""
        cubes = np.asarray(cubes, dtype=np.float64).reshape(self.nb, 7)
        best = np.inf
        for a, b, r, st in self.capsules_world(q):
            n = int(np.ceil(np.linalg.norm(b - a) / SPACING)) + 1
            P = a + np.linspace(0.0, 1.0, n)[:, None] * (b - a)
            for k in range(self.nb):
                best = min(best, point_box_distance(P, cubes[k, :3], quat2mat(cubes[k, 3:7]), self.box_half).min() - r)
        return best


def host_statics(task):
    """The engine's static boxes of `task` from the host build (tests/hostcheck/link_guard_check.py)."""
    from d3il_amd.model import blob as blob_mod
    from tests.hostcheck.link_guard_check import LinkGuardHost
    g = LinkGuardHost(blob_mod.load(task))
    return g.st_c, g.st_h, g.st_R


def reference(task):
    return GuardReference(task, host_statics(task))


# ---------------------------------------------------------------------------------------------------------------------------------------
# The scripted approach of the GPU tests (G1, G2), checked step by step against the reference.  The vertical rod reaches the table long before
# the fingers reach anything, so the hand is first TILTED (75 degrees about the world x axis, 1.5 degrees per step, the set-point rising 6 cm
# meanwhile: the rod then points sideways, its tip 3 cm below the TCP and 12 cm beside it), then carried over the target at 4 mm per step and
# lowered at 3 mm per step until the bit is set, then raised again for RISE steps.

BIT = 1 << 20
BAD = (1 << 16) | (1 << 18) | (1 << 19)
TILT, RISE = 75.0, 12


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def drive_descent(ref, step, state0, targets, slack, max_steps=330):
    """step(actions [n, 7]) -> (state [rows, n], flags [n]) runs one env step; state0: the state after the reset; targets [n, 2]: where each environment's
    hand goes down.  Asserts per step and environment: bit clear while every reference distance so far was > margin + slack + 1 mm, bit set from the first
    step at which one was < margin - 1 mm; state finite, none of the bits 16 / 18 / 19.  Returns per environment a dict: step at which the bit was first
    seen, the reference's (distance, pair) and capsule <-> cube distance at that step, the reference distance at the end (hand raised again)."""
    n = targets.shape[0]
    m = ref.margin
    des = state0[25:28].T.copy()
    may, must = np.zeros(n, bool), np.zeros(n, bool)
    seen = [None] * n
    last = np.zeros(n)
    for t in range(max_steps):
        th = np.deg2rad(min(TILT, 1.5 * (t + 1)))
        quat = _qmul(np.array([np.cos(th / 2), np.sin(th / 2), 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0]))
        for e in range(n):
            if t < 50:
                des[e, 2] += 0.0012
                continue
            v = targets[e] - des[e, :2]
            dist = np.linalg.norm(v)
            if dist > 1e-9:
                des[e, :2] += v / dist * min(dist, 0.004)
            elif seen[e] is None:
                des[e, 2] -= 0.003      # the descent stops as soon as the bit is set
            else:
                des[e, 2] += 0.003
        st, fl = step(np.concatenate([des, np.tile(quat, (n, 1))], axis=1))
        assert np.isfinite(st).all(), "state not finite at step %d" % t
        assert not (fl & BAD).any(), "divergence flags %s at step %d" % ([hex(int(f)) for f in fl & BAD], t)
        for e in range(n):
            cubes = st[42:42 + 13 * ref.nb, e].reshape(ref.nb, 13)[:, :7]
            d, who = ref.distance(st[:9, e], cubes)
            last[e] = d
            may[e] |= d <= m + slack + 1e-3
            must[e] |= d < m - 1e-3
            bit = bool(fl[e] & BIT)
            assert bit or not must[e], "env %d step %d: reference distance %.5f < margin - 1 mm (%s) but the bit is clear" % (e, t, d, who)
            assert may[e] or not bit, "env %d step %d: bit set although every reference distance so far was > margin + slack + 1 mm (now %.5f, %s)" % (e, t, d, who)
            if bit and seen[e] is None:
                seen[e] = dict(step=t, d=d, who=who, cube_d=ref.cube_distance(st[:9, e], cubes))
        if all(s is not None and t >= s["step"] + RISE for s in seen):
            break
    for e in range(n):
        assert seen[e] is not None and must[e], "env %d: the hand never came below the margin (last reference distance %.4f)" % (e, last[e])
        seen[e]["d_end"] = last[e]
    return seen


def wall_target(ref, ctx_xy):
    """The static box to lower the wrist over: it stands at least 2 cm above the table top inside the arm's reach, is no slab, and is the one farthest (xy) from
    the cubes of the context."""
    top = ref.st_c[:, 2] + ref.st_h[:, 2]
    best = None
    for s in range(len(ref.st_c)):
        c = ref.st_c[s]
        if top[s] < top[0] + 0.02 or not (0.3 <= c[0] <= 0.7 and abs(c[1]) <= 0.45) or ref.st_h[s].max() > 0.3:
            continue
        far = np.linalg.norm(ctx_xy - c[:2], axis=1).min()
        if best is None or far > best[0]:
            best = (far, s)
    return best[1], ref.st_c[best[1], :2].copy()
