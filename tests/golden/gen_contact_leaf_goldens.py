"""Writes tests/golden/contact_leaf_box.npz and contact_leaf_rest.npz: the problems of tests/contact_leaf_cases.py (built from seeds) with their references.

    python tests/golden/gen_contact_leaf_goldens.py        (needs mpmath and the oracle library; under a minute)

Runs on the CPU, uses mpmath (40 digits), numpy (the yardsticks) and the oracle's colliders only - never the code under test.  The same run gives the same
bytes (fixed archive timestamps).  Families: see the lists below; what each reference is: the docstring of tests/contact_leaf_cases.py.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as orc            # noqa: E402
from tests import contact_leaf_cases as K   # noqa: E402

NALT = 6
NPERT = 16


def save(path, out):
    """np.savez_compressed with fixed archive timestamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(out):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(out[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, b.getvalue())
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s (%d bytes)" % (path, len(buf.getvalue())))


def blobs():
    d = os.path.join(ROOT, "d3il_amd", "model", "blobs")
    out = {}
    for f in sorted(os.listdir(d)):
        j = json.load(open(os.path.join(d, f)))
        if isinstance(j, dict) and "geoms" in j:
            out[f[:-5]] = j
    return out


def quat(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])


def rq(rng):
    q = rng.standard_normal(4)
    return q / np.linalg.norm(q)


def logu(rng, a, b):
    return float(np.exp(rng.uniform(np.log(a), np.log(b))))


def pack(names, fams, keys):
    """fams: list of lists of dicts -> {key: stacked array}, names, start."""
    out = {"names": np.array(names), "start": np.concatenate([[0], np.cumsum([len(f) for f in fams])]).astype(np.int64)}
    flat = [c for f in fams for c in f]
    for k in keys:
        out[k] = np.array([c[k] for c in flat])
    return out


# ================================================================================================ box_box
def oracle_answers(p1, q1, s1, p2, q2, s2, margin, rng):
    """(ordered answer on the input as given, list of distinct answers as sets over the input and NPERT perturbed copies)."""
    first = orc.box_box(p1, q1, s1, p2, q2, s2, margin=margin).copy()
    alts = [first]
    for _ in range(NPERT):
        v = [np.asarray(a, float) * (1 + 1e-15 * rng.standard_normal(len(a))) for a in (p1, q1, s1, p2, q2, s2)]
        v[1], v[4] = v[1] / np.linalg.norm(v[1]), v[4] / np.linalg.norm(v[4])
        r = orc.box_box(*v, margin=margin).copy()
        if not any(K.same_set(r, len(r), a, len(a)) for a in alts):
            alts.append(r)
    return first, alts


def box_case(p1, q1, s1, p2, q2, s2, margin, rng):
    c = dict(p1=np.asarray(p1, float), R1=K.quat2mat_np(q1), s1=np.asarray(s1, float), p2=np.asarray(p2, float), R2=K.quat2mat_np(q2), s2=np.asarray(s2, float), margin=float(margin))
    for pre, a in (("", (p1, q1, s1, p2, q2, s2)), ("sw_", (p2, q2, s2, p1, q1, s1))):
        first, alts = oracle_answers(*a, margin, rng)
        if len(alts) > NALT:
            return None
        rec, arec, an = np.zeros((8, 7)), np.zeros((NALT, 8, 7)), np.zeros(NALT, dtype=np.int32)
        rec[:len(first)] = first
        for k, a_ in enumerate(alts):
            arec[k, :len(a_)] = a_
            an[k] = len(a_)
        c.update({pre + "ref_count": np.int32(len(first)), pre + "ref_rec": rec, pre + "alt_num": np.int32(len(alts)), pre + "alt_count": an, pre + "alt_rec": arec})
    return c


def on_top(rng, s1, s2, yaw1, yaw2, tilt, gap, off):
    """Box 2 lying on box 1's +z face: (p1, q1, p2, q2)."""
    q1 = quat([0, 0, 1], yaw1)
    q2 = qmul(quat(rng.standard_normal(3), tilt) if tilt else np.array([1.0, 0, 0, 0]), quat([0, 0, 1], yaw2))
    p1 = rng.uniform(-0.1, 0.1, 3)
    return p1, q1, p1 + np.array([off[0], off[1], s1[2] + s2[2] + gap]), q2


def sat_edge_vs_face(p1, q1, s1, p2, q2, s2):
    """(best face separation, best edge separation) of the 15 axes in f64 - to place a pose at the FUDGE rule's threshold."""
    ax, sep = K.box_axes_separation(p1, K.quat2mat_np(q1), s1, p2, K.quat2mat_np(q2), s2)
    return sep[:6].max(), (sep[6:].max() if len(sep) > 6 else -np.inf)


def box_families(B):
    rng = np.random.default_rng(20251)
    cube = np.array([0.025, 0.025, 0.025])
    task_sizes = sorted({tuple(g["size"]) for b in B.values() for g in b["geoms"] if g.get("type") == "box"})
    cubes = [np.array(s) for s in task_sizes if max(s) <= 0.05 and min(s) >= 0.02]
    tips = [np.array(s) for s in task_sizes if max(s) <= 0.008]
    slabs = [np.array(s) for s in task_sizes if s[0] >= 0.3 and s[1] >= 0.3]
    beams = [np.array(s) for s in task_sizes if sorted(s)[1] <= 0.02 and max(s) >= 0.4]
    assert cubes and tips and slabs and beams, (cubes, tips, slabs, beams)
    fams = {}

    def fill(name, make, n=32, stable=True):
        got, dropped, tries = [], 0, 0
        while len(got) < n:
            tries += 1
            assert tries < 40 * n, name
            a = make(len(got))
            if a is None:
                continue
            c = box_case(*a, rng)
            if c is None or (stable and (c["alt_num"] > 1 or c["sw_alt_num"] > 1)):
                dropped += 1
                continue
            got.append(c)
        if stable:
            assert dropped <= 0.05 * (len(got) + dropped), "%s: %d of %d candidates unstable" % (name, dropped, len(got) + dropped)
        cnt = np.bincount([int(c["ref_count"]) for c in got], minlength=9)
        print("box_box %-22s %d cases, %d dropped, counts %s, tie cases %d" % (name, len(got), dropped, list(cnt), sum(int(c["alt_num"]) > 1 for c in got)))
        fams[name] = got

    def random_pose(k):
        s1, s2 = rng.uniform(0.02, 0.06, 3), rng.uniform(0.02, 0.06, 3)
        p1 = rng.uniform(-0.1, 0.1, 3)
        return p1, rq(rng), s1, p1 + rng.uniform(-0.07, 0.07, 3), rq(rng), s2, 0.0
    fill("random", random_pose, 48)

    def flat(tilt_max):
        def make(k):
            s1 = rng.uniform(0.02, 0.06, 3) if k % 4 else np.array([0.03, 0.03, 0.03])
            s2 = rng.uniform(0.02, 0.06, 3) if k % 4 else np.array([0.03, 0.05, 0.03])
            if k % 5 == 0:
                s2 = s1.copy()
            p1, q1, p2, q2 = on_top(rng, s1, s2, rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi), rng.uniform(0, tilt_max) if tilt_max else 0.0,
                                    rng.uniform(-0.004, 0.0015), rng.uniform(-0.05, 0.05, 2))
            return p1, q1, s1, p2, q2, s2, [0.0, 0.001, 0.002][k % 3]
        return make
    fill("flat_tilt", flat(0.05), 48)
    fill("flat_no_tilt", flat(0.0))

    def equal_faces(k):      # finger tips on each other, identical cubes stacked: same yaw, no offset
        s = [tips[k % len(tips)], cubes[k % len(cubes)], cube][k % 3]
        yaw = rng.uniform(-np.pi, np.pi)
        p1, q1, p2, q2 = on_top(rng, s, s, yaw, yaw, 0.0, -logu(rng, 1e-6, 2e-3), (0.0, 0.0))
        return p1, q1, s, p2, q1.copy(), s, [0.0, 0.001][k % 2]
    fill("equal_faces", equal_faces)

    def slab(k):             # a small cube on a slab 10 - 20 times its size: axis-aligned and at yaw 0, pi / 2, random (both geom orders: the sw_ references)
        s2 = cube * rng.uniform(0.8, 1.2)
        s1 = np.array([s2[0] * rng.uniform(10, 20), s2[0] * rng.uniform(10, 20), s2[0] * rng.uniform(0.04, 4)])
        yaw = [0.0, np.pi / 2, rng.uniform(-np.pi, np.pi), 0.0][k % 4]
        p1, q1, p2, q2 = on_top(rng, s1, s2, 0.0, yaw, 0.0, -logu(rng, 1e-6, 1e-3), rng.uniform(-0.1, 0.1, 2))
        if k % 4 == 3:
            p1 = np.zeros(3)
            p2 = np.array([0.05, -0.025, s1[2] + s2[2] - 0.0005])
        return p1, q1, s1, p2, q2, s2, 0.0
    fill("slab", slab)

    def hair(k):             # a hair apart, inside the margin
        s1, s2 = rng.uniform(0.02, 0.06, 3), rng.uniform(0.02, 0.06, 3)
        margin = [0.001, 0.002][k % 2]
        p1, q1, p2, q2 = on_top(rng, s1, s2, rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi), [0.0, 1e-3][k % 2] * rng.uniform(0, 1),
                                logu(rng, 1e-7, 0.9 * margin), rng.uniform(-0.03, 0.03, 2))
        return p1, q1, s1, p2, q2, s2, margin
    fill("hair_apart", hair)

    def task(k):             # the half sizes the tasks use, in the poses they rest in
        kind = k % 4
        if kind == 0:        # cube on a table slab
            s1, s2 = slabs[k // 4 % len(slabs)], cubes[k // 4 % len(cubes)]
            p1, q1, p2, q2 = on_top(rng, s1, s2, 0.0, rng.uniform(-np.pi, np.pi), 0.0, -logu(rng, 1e-6, 1e-4), rng.uniform(-0.2, 0.2, 2))
        elif kind == 1:      # cube pushed against a frame beam
            s1, s2 = beams[k // 4 % len(beams)], cubes[k // 4 % len(cubes)]
            ax = int(np.argmin(s1[:2])) if s1[2] < 0.1 else 0
            p1, q1 = rng.uniform(-0.1, 0.1, 3), np.array([1.0, 0, 0, 0])
            off = np.zeros(3)
            off[ax] = s1[ax] + s2[ax] - logu(rng, 1e-5, 1e-3)
            off[1 - ax if s1[2] < 0.1 else 2] = rng.uniform(-0.3, 0.3)
            p2, q2 = p1 + off, quat([0, 0, 1], rng.uniform(-0.3, 0.3))
        elif kind == 2:      # finger tip on a cube's side
            s1, s2 = cubes[k // 4 % len(cubes)], tips[0]
            p1, q1 = rng.uniform(-0.1, 0.1, 3), quat([0, 0, 1], rng.uniform(-np.pi, np.pi))
            R = K.quat2mat_np(q1).reshape(3, 3)
            p2 = p1 + R @ np.array([0, s1[1] + s2[1] - logu(rng, 1e-5, 5e-4), rng.uniform(-0.01, 0.01)])
            q2 = qmul(q1, quat([0, 0, 1], rng.uniform(-0.05, 0.05)))
        else:                # two task cubes side by side
            s1, s2 = cubes[k // 4 % len(cubes)], cubes[(k // 4 + 1) % len(cubes)]
            p1, q1 = rng.uniform(-0.1, 0.1, 3), quat([0, 0, 1], rng.uniform(-np.pi, np.pi))
            q2 = quat([0, 0, 1], rng.uniform(-np.pi, np.pi))
            d = rng.uniform(-1, 1, 2)
            d /= np.linalg.norm(d)
            p2 = p1 + np.array([*(d * rng.uniform(0.04, 0.075)), s2[2] - s1[2]])
        return p1, q1, s1, p2, q2, s2, 0.0
    fill("task_sizes", task)

    def near_parallel(k):    # edges nearly parallel: 1 - Cm^2 = sin^2(theta) in [1e-11, 1e-6], both sides of the routine's 1e-10 skip
        s1, s2 = rng.uniform(0.02, 0.06, 3), rng.uniform(0.02, 0.06, 3)
        th = np.sqrt(logu(rng, 1e-11, 1e-6)) if k % 2 else np.sqrt(1e-10 * (1 + [-1, 1][k // 2 % 2] * logu(rng, 1e-6, 0.5)))
        h = rng.uniform(-1, 1, 2)
        q1 = quat([0, 0, 1], rng.uniform(-np.pi, np.pi))
        q2 = qmul(q1, quat([h[0], h[1], 0.0], th))
        p1 = rng.uniform(-0.1, 0.1, 3)
        R = K.quat2mat_np(q1).reshape(3, 3)
        p2 = p1 + R @ np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), s1[2] + s2[2] - logu(rng, 1e-5, 2e-3)])
        return p1, q1, s1, p2, q2, s2, 0.0
    fill("near_parallel", near_parallel)

    # ---- tie families: knife edges on purpose, no cap on the share of tie cases
    def cubes45(k):          # equal cubes side by side at exactly 45 degrees of relative yaw: the two candidate incident faces tie
        s = [cube, np.array([0.03, 0.03, 0.03])][k % 2]
        yaw = [0.0, np.pi / 2, rng.uniform(-np.pi, np.pi)][k % 3]
        q1, q2 = quat([0, 0, 1], yaw), quat([0, 0, 1], yaw + np.pi / 4)
        R = K.quat2mat_np(q1).reshape(3, 3)
        p1 = [np.zeros(3), rng.uniform(-0.1, 0.1, 3)][k % 2]
        p2 = p1 + R @ np.array([s[0] * (1 + np.sqrt(2)) - logu(rng, 1e-5, 2e-3), [0.0, rng.uniform(-0.01, 0.01)][k // 2 % 2], 0.0])
        return p1, q1, s, p2, q2, s, 0.0
    fill("tie_cubes_45", cubes45, stable=False)

    def face_band(k):        # the two boxes' face-axis separations tied inside the 1e-10 band; equal and unequal face areas
        s1 = rng.uniform(0.02, 0.06, 3)
        s2 = s1.copy() if k % 2 else rng.uniform(0.02, 0.06, 3)
        tilt = [0.0, logu(rng, 1e-9, 1e-6)][k // 2 % 2]
        p1, q1, p2, q2 = on_top(rng, s1, s2, rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi), tilt, -logu(rng, 1e-5, 2e-3), rng.uniform(-0.03, 0.03, 2))
        return p1, q1, s1, p2, q2, s2, 0.0
    fill("tie_face_band", face_band, stable=False)

    def edge_fudge(k):       # an edge axis within the FUDGE factor (1.05) of the best face axis: crossed edges, turned until FUDGE x edge = face, then 0, +-1e-15 .. 1e-9 off
        s1, s2 = rng.uniform(0.025, 0.04, 3), rng.uniform(0.025, 0.04, 3)
        q1 = quat([1, 0, 0], np.pi / 4)
        pen = logu(rng, 5e-4, 3e-3)
        p1 = np.zeros(3)

        def pose(a):
            q2 = qmul(quat([0, 0, 1], rng_yaw), quat([0, 1, 0], a))
            R1, R2 = K.quat2mat_np(q1).reshape(3, 3), K.quat2mat_np(q2).reshape(3, 3)
            top1 = np.abs(R1[2]) @ s1
            bot2 = np.abs(R2[2]) @ s2
            return np.array([0.0, 0.0, top1 + bot2 - pen]), q2
        rng_yaw = rng.uniform(-0.2, 0.2)

        def f(a):
            p2, q2 = pose(a)
            fb, eb = sat_edge_vs_face(p1, q1, s1, p2, q2, s2)
            return eb * 1.05 - fb
        grid = np.linspace(0.02, np.pi / 4, 60)
        vals = [f(a) for a in grid]
        idx = [i for i in range(len(grid) - 1) if vals[i] * vals[i + 1] < 0]
        if not idx:
            return None
        lo, hi = grid[idx[0]], grid[idx[0] + 1]
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if f(lo) * f(mid) <= 0:
                hi = mid
            else:
                lo = mid
        a = lo * (1 + [0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6][k % 8])
        p2, q2 = pose(a)
        return p1, q1, s1, p2, q2, s2, 0.0
    fill("tie_edge_fudge", edge_fudge, stable=False)
    names = list(fams)
    keys = ["p1", "R1", "s1", "p2", "R2", "s2", "margin"] + [pre + k for pre in ("", "sw_") for k in ("ref_count", "ref_rec", "alt_num", "alt_count", "alt_rec")]
    return pack(names, [fams[n] for n in names], keys)


# ================================================================================================ cyl_box
RODS = ((0.01, 0.15), (0.025, 0.1), (0.03, 0.07))      # radius, half length of the tasks' rods and pegs


def cyl_families():
    rng = np.random.default_rng(20252)
    fams = {}

    def case(pc, qc, rad, half, pb, qb, sb, margin):
        axis = K.quat2mat_np(qc).reshape(3, 3)[:, 2].copy()
        return case_axis(pc, axis, rad, half, pb, qb, sb, margin, qc)

    def case_axis(pc, axis, rad, half, pb, qb, sb, margin, qc=None):
        Rb = K.quat2mat_np(qb)
        r = K.cyl_reference(pc, axis, rad, half, pb, Rb, sb, margin)
        if r["gap"] < 1e-9 or (r["through"] and r["depth_gap"] < 1e-9) or r["through_gap"] < 0.9e-9:
            return None
        c = dict(pc=np.asarray(pc, float), axis=np.asarray(axis, float), par=np.array([rad, half, margin]), pb=np.asarray(pb, float), Rb=Rb, sb=np.asarray(sb, float),
                 ref_hit=np.int32(r["hit"]), ref_dist=r["dist"], ref_out=r["out"], through=np.int32(r["through"]), dmin=r["dmin"], tm=r["tm"], tp=r["tp"],
                 orc_hit=np.int32(0), orc_out=np.zeros(7))
        if qc is not None:
            o = orc.cyl_box(pc, qc, rad, half, pb, qb, sb, margin=margin)
            if o is not None:
                c["orc_hit"], c["orc_out"] = np.int32(1), o.copy()
        return c

    def fill(name, make, n=24):
        got = []
        while len(got) < n:
            c = make(len(got))
            if c is not None:
                got.append(c)
        print("cyl_box %-14s %d cases, hits %d, through %d" % (name, n, sum(int(c["ref_hit"]) for c in got), sum(int(c["through"]) for c in got)))
        fams[name] = got

    def random_pose(k):
        rad, half = RODS[k % 3]
        sb, pb = rng.uniform(0.02, 0.05, 3), rng.uniform(-0.1, 0.1, 3)
        return case(pb + rng.uniform(-0.08, 0.08, 3), rq(rng), rad, half, pb, rq(rng), sb, 0.02)
    fill("random", random_pose, 48)

    def upright(k):          # the task regime: upright rod by a yawed upright cube, u[i] exactly 0
        rad, half = RODS[k % 3]
        sb, pb = rng.uniform(0.02, 0.05, 3), rng.uniform(-0.1, 0.1, 3)
        qb = quat([0, 0, 1], rng.uniform(-np.pi, np.pi))
        return case(pb + np.array([*rng.uniform(-0.08, 0.08, 2), rng.uniform(0.0, 0.14)]), np.array([0.0, 1, 0, 0]), rad, half, pb, qb, sb, [0.0, 0.02][k % 2])
    fill("upright", upright, 32)

    def tiny_u(k):           # |u[i]| on both sides of 1e-14
        rad, half = RODS[k % 3]
        sb, pb = rng.uniform(0.02, 0.05, 3), rng.uniform(-0.1, 0.1, 3)
        qb = quat([0, 0, 1], [0.0, rng.uniform(-np.pi, np.pi)][k % 2])
        t = rng.uniform(-1, 1, 2)
        t *= logu(rng, 1e-15, 1e-13) / np.linalg.norm(t) if k % 4 < 2 else [0.5e-14, 2e-14][k % 2] / np.linalg.norm(t)
        axis = np.array([t[0], t[1], 1.0])
        return case_axis(pb + np.array([*rng.uniform(-0.08, 0.08, 2), rng.uniform(0.0, 0.14)]), axis / np.linalg.norm(axis), rad, half, pb, qb, sb, 0.02)
    fill("tiny_u", tiny_u)

    def end_beside(k):       # a rod end beside the box: caps are not modelled, the end point clamps
        rad, half = RODS[k % 3]
        sb, pb, qb, qc = rng.uniform(0.02, 0.05, 3), rng.uniform(-0.1, 0.1, 3), rq(rng), rq(rng)
        axis = K.quat2mat_np(qc).reshape(3, 3)[:, 2]
        side = rng.standard_normal(3)
        side -= (side @ axis) * axis
        side /= np.linalg.norm(side)
        pc = pb + axis * (half + np.linalg.norm(sb) * rng.uniform(0.2, 1.0)) * [-1, 1][k % 2] + side * rng.uniform(0, 0.03)
        return case(pc, qc, rad, half, pb, qb, sb, 0.05)
    fill("end_beside", end_beside)

    def over(corner):
        def make(k):         # a lying rod over an edge / a corner of the box: the nearest box point is on that edge / is that corner
            rad, half = RODS[k % 3]
            sb, pb, qb = rng.uniform(0.02, 0.05, 3), rng.uniform(-0.1, 0.1, 3), rq(rng)
            Rb = K.quat2mat_np(qb).reshape(3, 3)
            sg = rng.choice([-1.0, 1.0], 3)
            if corner:
                out, pt = sg / np.sqrt(3), sg * sb
            else:
                e = k % 3
                out = sg.copy()
                out[e] = 0
                out /= np.sqrt(2)
                pt = sg * sb
                pt[e] = rng.uniform(-0.8, 0.8) * sb[e]
            out = out + 0.2 * rng.standard_normal(3) * np.abs(out)      # (stays in the outward cone of the feature)
            out /= np.linalg.norm(out)
            u = np.cross(out, rng.standard_normal(3))
            u /= np.linalg.norm(u)
            x = pt + out * (rad + rng.uniform(-0.004, 0.01)) + u * rng.uniform(-0.5, 0.5) * half
            z = np.array([0.0, 0, 1])
            ua = Rb @ u
            v = np.cross(z, ua)
            qc = quat(v if np.linalg.norm(v) > 1e-9 else [1, 0, 0], np.arccos(np.clip(ua[2], -1, 1)))
            return case(pb + Rb @ x, qc, rad, half, pb, qb, sb, 0.005)
        return make
    fill("over_edge", over(False))
    fill("over_corner", over(True))

    def through(k):
        rad, half = RODS[k % 3]
        sb, pb = rng.uniform(0.02, 0.05, 3), rng.uniform(-0.1, 0.1, 3)
        qb = rq(rng)
        qc = [rq(rng), np.array([0.0, 1, 0, 0])][k % 2]
        if k % 2:
            qb = quat([0, 0, 1], rng.uniform(-np.pi, np.pi))
        Rb = K.quat2mat_np(qb).reshape(3, 3)
        axis = K.quat2mat_np(qc).reshape(3, 3)[:, 2]
        return case(pb + Rb @ (rng.uniform(-0.9, 0.9, 3) * sb) + axis * rng.uniform(-0.5, 0.5) * half, qc, rad, half, pb, qb, sb, 0.0)
    fill("through", through)

    def margin_edge(k):      # dist within 1e-6 of the margin, either side (never closer than 1e-9)
        rad, half = RODS[k % 3]
        sb, pb = rng.uniform(0.02, 0.05, 3), rng.uniform(-0.1, 0.1, 3)
        yaw = [0.0, rng.uniform(-np.pi, np.pi)][k % 2]
        qb = quat([0, 0, 1], yaw)
        margin = [0.0, 0.001, 0.02][k % 3]
        off = logu(rng, 2e-9, 1e-6) * [-1, 1][k // 3 % 2]
        Rb = K.quat2mat_np(qb).reshape(3, 3)
        x = np.array([sb[0] + rad + margin + off, rng.uniform(-0.8, 0.8) * sb[1], rng.uniform(0, 0.1)])
        return case(pb + Rb @ x, np.array([0.0, 1, 0, 0]), rad, half, pb, qb, sb, margin)
    fill("margin_edge", margin_edge)

    def cull(k):             # the cull radius of gen_phase3: the cube's centre at |box_half| + rod_r from the rod's segment, +-1e-3 relative; margin 0 as there
        rad, half = RODS[0]
        sb = np.array([0.025, 0.025, 0.025]) if k % 2 else rng.uniform(0.02, 0.05, 3)
        pb, qb, qc = rng.uniform(-0.1, 0.1, 3), rq(rng), rq(rng)
        axis = K.quat2mat_np(qc).reshape(3, 3)[:, 2]
        side = rng.standard_normal(3)
        side -= (side @ axis) * axis
        side /= np.linalg.norm(side)
        rr = (np.linalg.norm(sb) + rad) * (1 + rng.uniform(-1e-3, 1e-3))
        t = rng.uniform(-1.2, 1.2) * half
        beyond = max(abs(t) - half, 0.0)
        lat = np.sqrt(max(rr * rr - beyond * beyond, 0.0))
        return case(pb - axis * t - side * lat, qc, rad, half, pb, qb, sb, 0.0)
    fill("cull", cull)
    names = list(fams)
    return pack(names, [fams[n] for n in names], ["pc", "axis", "par", "pb", "Rb", "sb", "ref_hit", "ref_dist", "ref_out", "through", "dmin", "tm", "tp", "orc_hit", "orc_out"])


# ================================================================================================ cone
def cone_families(B):
    rng = np.random.default_rng(20253)
    frics = sorted({g["friction"][0] for b in B.values() for g in b["geoms"]})
    mu_scale = float(np.sqrt(1 / K.IMPRATIO))
    fams = {}

    def params(k, fric=None):
        fric = frics[k % len(frics)] if fric is None else fric
        Dn = logu(rng, 1e2, 1e6)
        return Dn, Dn * K.IMPRATIO, fric * mu_scale, fric      # as gen_solve / gen_tree call the routine

    def case(jar, Dn, Dt, mu, fric, edge=False, hess=True):
        jar = np.asarray(jar, float)
        ref, zone = K.cone_reference(jar, Dn, Dt, mu, fric)
        alt = ref[4:].copy()
        if edge:             # the Hessian of the zone across the boundary
            N, T = jar[0] * mu, np.hypot(jar[1], jar[2]) * fric
            other = {0: 2, 1: 2, 2: 0 if abs(N - mu * T) < abs(mu * N + T) else 1}[zone]
            alt = K.cone_reference(jar, Dn, Dt, mu, fric, zone=other)[0][4:]
        return dict(jar=jar, par=np.array([Dn, Dt, mu, fric]), ref=ref, alt=alt, zone=np.int32(zone), edge=np.int32(edge), hess=np.int32(hess),
                    yard=K.cone_numpy(jar, Dn, Dt, mu, fric))

    def tangent(lo=1e-4, hi=1e-1):
        a = rng.uniform(0, 2 * np.pi)
        T = logu(rng, lo, hi)
        return T, np.array([np.cos(a), np.sin(a)]) * T

    def interior(zone):
        def make(k):
            Dn, Dt, mu, fric = params(k)
            T, t = tangent()             # T = |U| = fric |jar tangential|
            if zone == 0:
                j0 = T * rng.uniform(1.05, 5)
            elif zone == 1:
                j0 = -T / mu ** 2 * rng.uniform(1.05, 5)
            else:
                j0 = rng.uniform(-0.95 * T / mu ** 2, 0.95 * T)
            return case([j0, t[0] / fric, t[1] / fric], Dn, Dt, mu, fric)
        return make

    def boundary(delta, top):
        def make(k):         # a boundary from both sides: N = mu T (1 +- delta) (top) or N = -(T / mu) (1 +- delta) (bottom)
            Dn, Dt, mu, fric = params(k)
            T, t = tangent()
            j0 = (T if top else -T / mu ** 2) * (1 + [-1, 1][k % 2] * delta)
            return case([j0, t[0] / fric, t[1] / fric], Dn, Dt, mu, fric, edge=delta < 1e-12)
        return make
    n = 24
    fams["top"] = [interior(0)(k) for k in range(n)]
    fams["bottom"] = [interior(1)(k) for k in range(n)]
    fams["middle"] = [interior(2)(k) for k in range(n)]
    for d in (1e-3, 1e-9, 1e-15):      # (a family per boundary: at the top one the cost goes to zero and its relative error is the cancellation's, at the bottom one not)
        fams["top_edge_%g" % d] = [boundary(d, True)(k) for k in range(16)]
        fams["bottom_edge_%g" % d] = [boundary(d, False)(k) for k in range(16)]
    fams["T_zero"] = [case([[-1, 1][k % 2] * logu(rng, 1e-6, 1e-1), 0.0, 0.0], *params(k)) for k in range(12)]
    fams["inert"] = [case(rng.standard_normal(3) * 0.01, 0.0, 0.0, *params(k)[2:]) for k in range(6)]

    def mu_small(k):         # mu -> 0: the fmax(1e-15, mu^2 (1 + mu^2)) guard takes over at mu = 3.2e-8
        mu = [1e-2, 1e-4, 1e-6, 1e-7, 4e-8, 2.5e-8, 1e-8, 1e-9][k % 8]
        Dn = logu(rng, 1e2, 1e6)
        fric = mu / mu_scale
        T, t = tangent()
        return case([T * rng.uniform(-0.5, 0.5), t[0] / fric, t[1] / fric], Dn, Dn * K.IMPRATIO, mu, fric)
    fams["mu_small"] = [mu_small(k) for k in range(n)]
    base = []
    # the apex: one set of residuals of order 1 (tangential part T in [0.1, 1]; 14 in the middle zone, one in each of the others), scaled down.  iT^3 leaves the
    # f64 range once T < 2e-103 and T^2 becomes subnormal below 1e-154: the scales 1e-105 .. 1e-150 lie inside that window for every member, 1e-100 outside it
    for k in range(16):
        Dn, Dt, mu, fric = params(k)
        if k == 0:           # (the residuals of the report: jar = (0, s, s / 2), Dn 1000, Dt 500, mu = fric = 1)
            base.append((np.array([0.0, 1.0, 0.5]), 1000.0, 500.0, 1.0, 1.0))
            continue
        T, t = tangent(0.1, 1.0)
        j0 = T * rng.uniform(1.05, 3) if k == 14 else (-T / mu ** 2 * rng.uniform(1.05, 3) if k == 15 else rng.uniform(-0.9 * T / mu ** 2, 0.9 * T))
        base.append((np.array([j0, t[0] / fric, t[1] / fric]), Dn, Dt, mu, fric))
    for sc in K.APEX_ASSERTED + K.APEX_RECORDED:
        fams["apex_%g" % sc] = [case(j * sc, *p, hess=sc in K.APEX_ASSERTED) for j, *p in base]
    names = list(fams)
    for nme in names:
        z = np.bincount([int(c["zone"]) + 1 for c in fams[nme]], minlength=4)
        print("cone %-16s %d cases, zones inert/top/bottom/middle %s" % (nme, len(fams[nme]), list(z)))
    return pack(names, [fams[n_] for n_ in names], ["jar", "par", "ref", "alt", "zone", "edge", "hess", "yard"])


# ================================================================================================ ldl
def ldl_families(n, seed):
    rng = np.random.default_rng(seed)
    tri = np.tril_indices(n)
    fams = {}

    def case(A, b):
        a = np.ascontiguousarray((0.5 * (A + A.T))[tri])
        ok, x, piv = K.ldl_reference(a, b, n)
        assert not np.any(np.abs(piv[piv != 0] / K.PIVOT_MIN - 1) < 1e-6)
        yard = np.full(n, np.nan)
        if ok:
            yard = K.ldl_numpy(a, b, n)
        return dict(A=a, b=np.asarray(b, float), ok=np.int32(ok), x=x, piv=piv, yard=yard)

    def orth():
        q, r = np.linalg.qr(rng.standard_normal((n, n)))
        return q * np.sign(np.diag(r))

    def spectral(cond, neg=False):
        Q = orth()
        e = logu(rng, 1e-2, 1e3) * np.exp(-np.log(cond) * np.sort(rng.uniform(0, 1, n)))
        e[0], e[-1] = e.max(), e.max() / cond
        if neg:
            e[rng.integers(n)] *= -rng.uniform(0.1, 1)
        return case((Q * e) @ Q.T, rng.standard_normal(n))
    m = 12
    for cond in (1.0, 1e4, 1e8, 1e12):
        fams["cond_%g" % cond] = [spectral(cond) for _ in range(m)]

    def schur():             # J D J' + mass, J = random contact rows (up to 3 contacts x 3 rows on the block's dofs)
        r = 3 * int(rng.integers(1, 4))
        J = rng.standard_normal((r, n)) * np.concatenate([np.ones(3), 0.03 * np.ones(n - 3)])
        D = np.array([logu(rng, 1e2, 1e6) for _ in range(r)])
        M = np.diag([logu(rng, 0.05, 0.5)] * 3 + [logu(rng, 1e-5, 1e-3) for _ in range(n - 3)])
        return case(J.T @ (D[:, None] * J) + M, rng.standard_normal(n))
    fams["schur"] = [schur() for _ in range(m)]
    fams["diagonal"] = [case(np.diag([logu(rng, 1e-6, 1e6) for _ in range(n)]), rng.standard_normal(n)) for _ in range(m)]

    def tiny(k):             # one pivot at 1e-300 (1 +- 1e-3), exactly: its row and column are otherwise zero
        j = int(rng.integers(n))
        keep = [i for i in range(n) if i != j]
        Q, r = np.linalg.qr(rng.standard_normal((n - 1, n - 1)))
        A = np.zeros((n, n))
        A[np.ix_(keep, keep)] = (Q * np.exp(rng.uniform(-2, 2, n - 1))) @ Q.T
        A[j, j] = 1e-300 * (1 + [-1e-3, 1e-3][k % 2])
        b = rng.standard_normal(n)
        b[j] = 1e-6 * rng.standard_normal()
        return case(A, b)
    fams["tiny_pivot"] = [tiny(k) for k in range(m)]
    fams["indefinite"] = [spectral(10.0 ** rng.uniform(0, 4), neg=True) for _ in range(m)]
    names = list(fams)
    for nme in names:
        print("ldl<%d> %-12s %d cases, ok %d" % (n, nme, len(fams[nme]), sum(int(c["ok"]) for c in fams[nme])))
    assert all(c["ok"] for nme in names if nme not in ("tiny_pivot", "indefinite") for c in fams[nme]) and not any(c["ok"] for c in fams["indefinite"])
    return pack(names, [fams[n_] for n_ in names], ["A", "b", "ok", "x", "piv", "yard"])


# ================================================================================================ cube_integrate
def cube_families(B):
    rng = np.random.default_rng(20255)
    ksub = sorted({b["n_substeps"] for b in B.values() if "n_substeps" in b} | {b["task_const"]["n_substeps"] for b in B.values() if "n_substeps" in b.get("task_const", {})})
    assert 35 in ksub, ksub
    h = K.TIMESTEP
    fams = {}

    def case(k, wmag, ang_acc=True, qscale=1.0):
        Kc = 1000 if k >= 6 else ksub[-1 - k % len(ksub)]
        q = rq(rng) * qscale
        w = rng.standard_normal(3)
        w *= wmag / max(np.linalg.norm(w), 1e-300)
        state = np.concatenate([rng.uniform(-0.5, 0.5, 3), q, rng.uniform(-0.5, 0.5, 3), w])
        acc = np.concatenate([rng.uniform(-10, 10, 3), rng.uniform(-20, 20, 3) * wmag / 50 if ang_acc else np.zeros(3)])
        return dict(state=state, acc=acc, h=h, K=np.int32(Kc), ref=K.cube_map_mp(state, acc, h, Kc), yard=K.cube_map_numpy(state, acc, h, Kc))
    m = 8
    fams["w_zero"] = [case(k, 0.0, ang_acc=False) for k in range(m)]
    fams["wh_below_1e-15"] = [case(k, 0.5e-15 / h, ang_acc=False) for k in range(m)]
    fams["wh_above_1e-15"] = [case(k, 2e-15 / h, ang_acc=False) for k in range(m)]
    for wm in (1.0, 50.0, 500.0):
        fams["w_%g" % wm] = [case(k, wm) for k in range(m)]
    fams["non_unit"] = [case(k, 5.0, qscale=[0.5, 2.0][k % 2]) for k in range(m)]
    names = list(fams)
    print("cube_integrate: %d families x %d cases, K = %s and 1000" % (len(names), m, ksub))
    return pack(names, [fams[n_] for n_ in names], ["state", "acc", "h", "K", "ref", "yard"])


# ================================================================================================ push_tan_yaw / quat2mat
def yaw_families():
    rng = np.random.default_rng(20256)
    fams = {}

    def case(q):
        q = np.asarray(q, float)
        t, R, cy = K.yaw_reference(q)
        return dict(q=q, tan=t, R=R, cy=cy, tan_yard=K.yaw_numpy(q), R_yard=K.quat2mat_np(q))
    m = 16
    fams["random"] = [case(rq(rng)) for _ in range(m)]
    fams["scale_0.5"] = [case(0.5 * rq(rng)) for _ in range(m)]
    fams["scale_2"] = [case(2.0 * rq(rng)) for _ in range(m)]
    fams["Nq_below_FEPS"] = [case(rq(rng) * [1e-9, 1e-10, 1.4e-8, 1e-20][k % 4]) for k in range(m)]
    fams["Nq_above_FEPS"] = [case(rq(rng) * [1.6e-8, 1e-7, 2e-8, 1e-6][k % 4]) for k in range(m)]
    gim = []
    while len(gim) < m:      # pitch of +-90 degrees: cy <= 4 FEPS
        c = case(qmul(qmul(quat([1, 0, 0], rng.uniform(-np.pi, np.pi)), quat([0, 1, 0], [-1, 1][len(gim) % 2] * np.pi / 2)), quat([0, 0, 1], rng.uniform(-np.pi, np.pi))))
        if c["cy"] <= 2 * K.FEPS:
            gim.append(c)
    fams["gimbal"] = gim
    for d in (1e-3, 1e-6, 1e-9):
        fams["near_90_%g" % d] = [case(qmul(quat([0, 0, 1], [-1, 1][k % 2] * (np.pi / 2 - d * rng.uniform(0.5, 1.5) * [-1, 1][k // 2 % 2])),
                                            quat(rng.standard_normal(3), [0.0, rng.uniform(0, 0.1)][k // 4 % 2]))) for k in range(m)]
    fams["yaw_0_pi"] = [case(q) for q in ([1.0, 0, 0, 0], [0.0, 0, 0, 1], [0.0, 0, 0, -1], [-1.0, 0, 0, 0], [2.0, 0, 0, 0], [0.0, 0, 0, 0.5], [-0.0, 0, 0, 1], [1.0, -0.0, -0.0, -0.0])]
    names = list(fams)
    for nme in names:
        print("tan_yaw %-14s %d cases, |tan| up to %.3g" % (nme, len(fams[nme]), max(abs(c["tan"]) for c in fams[nme])))
    return pack(names, [fams[n_] for n_ in names], ["q", "tan", "R", "cy", "tan_yard", "R_yard"])


def main():
    B = blobs()
    box = {"box__" + k: v for k, v in box_families(B).items()}
    save(K.NPZ_BOX, box)
    rest = {}
    for prefix, d in (("cyl", cyl_families()), ("cone", cone_families(B)), ("ldl5", ldl_families(5, 20254)), ("ldl6", ldl_families(6, 20264)), ("cube", cube_families(B)),
                      ("yaw", yaw_families())):
        rest.update({prefix + "__" + k: v for k, v in d.items()})
    save(K.NPZ_REST, rest)
    limit = max(os.path.getsize(os.path.join(os.path.dirname(K.NPZ_BOX), f)) for f in os.listdir(os.path.dirname(K.NPZ_BOX))
                if f.endswith(".npz") and not f.startswith("contact_leaf_"))
    for p in (K.NPZ_BOX, K.NPZ_REST):
        assert os.path.getsize(p) <= limit, "%s is larger than the largest other fixture (%d bytes)" % (p, limit)


if __name__ == "__main__":
    main()
