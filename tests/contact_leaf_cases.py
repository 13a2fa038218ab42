"""Problems, references, bounds and checkers of the contact engines' leaf routines (d3il_amd/csrc/rigid_common.h and their twins in gen_tree.h), shared by the
host suite (tests/test_contact_leaf_host.py) and the device suite (tests/test_gpu_contact_leaf.py).

tests/golden/contact_leaf_box.npz (box_box) and contact_leaf_rest.npz (written by tests/golden/gen_contact_leaf_goldens.py from seeds, mpmath at 40 digits and
the oracle's colliders; the code under test is never called there) hold per routine `<routine>__names` / `<routine>__start` (problems of family i: start[i] .. start[i + 1]) and its arrays.

box_box     inputs p, R (row-major), s of both boxes, margin.  From the oracle's array collider (an independent formulation of the same collider): the ordered
            answer on the input as stored, and `alts` = the distinct answers, as unordered contact sets, over the input and 16 copies perturbed by 1e-15
            relative (quaternions renormalised).  One alt: the case is STABLE - count and contacts are asserted in order at atol 1e-12 (the figure
            tests/test_push_kernel_host.py holds the host build to).  Families whose name starts with "tie_" are knife edges on purpose: the answer equals one
            of the alts as a set.  Every case: the geometric invariants of `box_box_invariants`, computed from the inputs alone.
cyl_box     the exact minimum of the segment <-> box distance (piecewise quadratic, convex: every breakpoint and every piece's stationary point) at 40 digits,
            and the minimising interval [tm, tp].  The routine's flatness rule is part of its definition: it scans g(t) = f'(t) / 2 over the sorted knots
            (segment ends, face-plane crossings) and counts a knot with |g| <= 1e-13 as stationary - for a strict minimum between two knots the interval is
            the exact root, for an axis that is parallel to a face (u[i] = 0 or |u[i]| of 1e-14) or passes through the box it is the whole flat stretch.
            The reference runs that scan in exact arithmetic; dist and the hit decision come from the minimum itself.  pos / normal are defined at the
            interval's midpoint.  Axis through the box (distance <= 1e-9): the routine's own
            definition, dist = -(smallest face depth at the midpoint) - rad.  atol 1e-12, the project's figure.
cone        cost = the zone-wise function of the header comment (top 0, bottom quadratic, middle Dm (N - mu T)^2 / 2), force = -d cost / d jar and
            Hc = d2 cost / d jar2 by mpmath differentiation of that cost.  Yardstick of a family: the error of `cone_numpy` (plain f64) against those values,
            relative to the largest entry of the quantity; bound 4 yardsticks (floored at 2^-52), the same for the twin.
ldl         mpmath LDL^T / solve; yardstick = a numpy-f64 Cholesky solve; ok == false exactly where a reference pivot is <= 1e-300.
cube        the discrete map of cube_integrate in mpmath, K calls; yardstick = the same map in numpy f64.
yaw         push_tan_yaw on the formula of geometric_transformation.py (quat2mat, mat2euler) and quat2mat (mju_quat2Mat) in mpmath; yardstick numpy f64.
"""
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPZ_BOX, NPZ_REST = os.path.join(_GOLDEN, "contact_leaf_box.npz"), os.path.join(_GOLDEN, "contact_leaf_rest.npz")
DIGITS = 40
FACTOR = 4.0
ULP = 2.0 ** -52
ATOL = 1e-12              # box_box / cyl_box against their references
FEPS = 2.220446049250313e-16
CYL_FLAT = 1e-13          # cyl_box's tolerance on g
CYL_THROUGH = 1e-9        # cyl_box: the axis counts as inside the box below this distance
PIVOT_MIN = 1e-300
IMPRATIO = 3.0            # every task blob's option.impratio
TIMESTEP = 0.001          # and timestep
YAW_FAMILIES = ("random", "scale_0.5", "scale_2", "Nq_below_FEPS", "Nq_above_FEPS", "gimbal", "near_90_0.001", "near_90_1e-06", "near_90_1e-09", "yaw_0_pi")
APEX_ASSERTED = (1.0, 1e-8, 1e-30, 1e-60, 1e-100)
APEX_RECORDED = (1e-105, 1e-120, 1e-150, 1e-170)      # cost and force asserted, finiteness of the Hessian recorded


def quat2mat_np(q):
    """mju_quat2Mat in numpy f64, row-major 9 (the generator's rotation matrices)."""
    w, x, y, z = (float(v) for v in q)
    return np.array([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z])


class Group:
    """One routine's arrays: g.<key>, g.names, g.rows(family), g.fam (family index per problem)."""

    def __init__(self, npz, prefix):
        self.names = [str(s) for s in npz[prefix + "__names"]]
        self.start = npz[prefix + "__start"]
        self.n = int(self.start[-1])
        self.fam = np.repeat(np.arange(len(self.names)), np.diff(self.start))
        for k in npz.files:
            if k.startswith(prefix + "__") and k not in (prefix + "__names", prefix + "__start"):
                setattr(self, k[len(prefix) + 2:], npz[k])

    def rows(self, name):
        i = self.names.index(name)
        return slice(int(self.start[i]), int(self.start[i + 1]))

    def fam_of(self, i):
        return self.names[self.fam[i]]


class Cases:
    def __init__(self):
        z = np.load(NPZ_REST)
        self.box = Group(np.load(NPZ_BOX), "box")
        self.cyl, self.cone, self.ldl5, self.ldl6, self.cube, self.yaw = (Group(z, p) for p in ("cyl", "cone", "ldl5", "ldl6", "cube", "yaw"))

        assert tuple(self.yaw.names) == YAW_FAMILIES

    def ldl(self, order):
        return self.ldl5 if order == 5 else self.ldl6


# ================================================================================================ box_box
def box_axes_separation(p1, R1, s1, p2, R2, s2):
    """The 15 candidate axes (unit; an edge pair that is parallel gives none) and the boxes' separation along each: (axes [m, 3], sep [m]), f64."""
    R1, R2 = np.asarray(R1, float).reshape(3, 3), np.asarray(R2, float).reshape(3, 3)
    d = np.asarray(p2, float) - np.asarray(p1, float)
    ax = [R1[:, i] for i in range(3)] + [R2[:, j] for j in range(3)]
    for i in range(3):
        for j in range(3):
            c = np.cross(R1[:, i], R2[:, j])
            l = np.linalg.norm(c)
            if l > 1e-5:                       # (1 - Cm^2 >= 1e-10, the routine's own skip)
                ax.append(c / l)
    ax = np.array(ax)
    return ax, np.array([separation_along(a, d, R1, s1, R2, s2) for a in ax])


def separation_along(n, d, R1, s1, R2, s2):
    """Gap between the two boxes' projections on the direction n (negative: overlap)."""
    R1, R2 = np.asarray(R1, float).reshape(3, 3), np.asarray(R2, float).reshape(3, 3)
    return abs(n @ d) - (np.abs(n @ R1) @ np.asarray(s1, float) + np.abs(n @ R2) @ np.asarray(s2, float))


def surface_distance(pt, p, R, s):
    """|distance| of a point from the surface of a box (0 on it), in long double."""
    x = np.asarray(R, np.longdouble).reshape(3, 3).T @ (np.asarray(pt, np.longdouble) - np.asarray(p, np.longdouble))
    e = np.abs(x) - np.asarray(s, np.longdouble)
    if (e <= 0).all():
        return float(-e.max())
    return float(np.sqrt((np.maximum(e, 0) ** 2).sum()))


def box_box_invariants(p1, R1, s1, p2, R2, s2, margin, cap, count, rec):
    """Violations (list of strings) of what geometry alone says about an answer; rec [8, 7] pre-filled with NaN by the caller.  Returns also the worst
    surface residual seen."""
    bad, worst = [], 0.0
    d = np.asarray(p2, float) - np.asarray(p1, float)
    ax, sep = box_axes_separation(p1, R1, s1, p2, R2, s2)
    if sep.max() > margin + 1e-13 and count != 0:
        bad.append("an axis separates the boxes by %.3e > margin %.3e but %d contacts" % (sep.max(), margin, count))
    if not 0 <= count <= min(cap, 8):
        bad.append("count %d outside [0, %d]" % (count, min(cap, 8)))
        return bad, worst
    if not np.isnan(rec[count:]).all():
        bad.append("rows past the count were written")
    if not np.isfinite(rec[:count]).all():
        bad.append("a contact row is not finite")
        return bad, worst
    for k in range(count):
        dist, pos, n = rec[k, 0], rec[k, 1:4], rec[k, 4:7]
        ln = float(np.sqrt((n.astype(np.longdouble) ** 2).sum()))
        if abs(ln - 1) > 1e-14:
            bad.append("contact %d: |normal| - 1 = %.2e" % (k, ln - 1))
        if n @ d < -1e-14:
            bad.append("contact %d: the normal points from box 2 to box 1 (n . d = %.3e)" % (k, n @ d))
        if not dist < margin:
            bad.append("contact %d: dist %.3e >= margin %.3e" % (k, dist, margin))
        r1 = surface_distance(pos - 0.5 * dist * n, p1, R1, s1)
        r2 = surface_distance(pos + 0.5 * dist * n, p2, R2, s2)
        worst = max(worst, r1, r2)
        if r1 > 1e-13 or r2 > 1e-13:
            bad.append("contact %d: surface points off the boxes by %.2e / %.2e" % (k, r1, r2))
        sn = separation_along(n, d, R1, s1, R2, s2)
        if dist < sn - 1e-13:
            bad.append("contact %d: dist %.6e below the separation along its normal %.6e" % (k, dist, sn))
    return bad, worst


def same_ordered(rec, count, ref, ref_count):
    return count == ref_count and (count == 0 or bool(np.abs(rec[:count] - ref[:count]).max() <= ATOL))


def same_set(rec, count, ref, ref_count):
    """Equal as unordered contact sets at ATOL (greedy matching: contacts of one answer are distinct by more than that)."""
    if count != ref_count:
        return False
    left = list(range(count))
    for k in range(count):
        hit = [j for j in left if np.abs(rec[k] - ref[j]).max() <= ATOL]
        if not hit:
            return False
        left.remove(hit[0])
    return True


def check_box(g, count, rec, label, cap=8, swapped=False):
    """count [n], rec [n, 8, 7] of every stored problem.  swapped: the answers are of the second geom order (box 2 first), compared with the `sw_` references.
    Prints one line per family; returns (violations, {family: [alt index taken per tie case]})."""
    pre = "sw_" if swapped else ""
    A, B = (("2", "1") if swapped else ("1", "2"))
    ref_n, ref_rec, alt_m, alt_n, alt_rec = (getattr(g, pre + k) for k in ("ref_count", "ref_rec", "alt_num", "alt_count", "alt_rec"))
    bad, taken = [], {}
    for name in g.names:
        s = g.rows(name)
        tie, worst_inv, worst_ref, unstable, in_order = name.startswith("tie_"), 0.0, 0.0, 0, 0
        hist = np.zeros(9, dtype=int)
        for i in range(s.start, s.stop):
            c, r = int(count[i]), rec[i]
            args = (getattr(g, "p" + A)[i], getattr(g, "R" + A)[i], getattr(g, "s" + A)[i], getattr(g, "p" + B)[i], getattr(g, "R" + B)[i], getattr(g, "s" + B)[i])
            inv, w = box_box_invariants(*args, g.margin[i], cap, c, r)
            worst_inv = max(worst_inv, w)
            bad += ["%s%s[%d]: %s" % (pre, name, i - s.start, m) for m in inv]
            if 0 <= c <= 8:
                hist[c] += 1
            if alt_m[i] > 1:
                unstable += 1
            if not tie:
                assert alt_m[i] == 1, "a stored case of a stable family has alternatives"
                if not same_ordered(r, c, ref_rec[i], ref_n[i]):
                    bad.append("%s%s[%d]: count %d (oracle %d) or a contact differs by more than %.0e, in order" % (pre, name, i - s.start, c, ref_n[i], ATOL))
                elif c:
                    worst_ref = max(worst_ref, np.abs(r[:c] - ref_rec[i][:c]).max())
            else:
                m = [a for a in range(alt_m[i]) if same_set(r, c, alt_rec[i, a], alt_n[i, a])]
                taken.setdefault(name, []).append(m[0] if m else -1)
                in_order += int(same_ordered(r, c, ref_rec[i], ref_n[i]))
                if not m:
                    bad.append("%s%s[%d]: %d contacts, none of the oracle's %d answers (counts %s)" % (pre, name, i - s.start, c, alt_m[i], list(alt_n[i, :alt_m[i]])))
        print("%-9s box_box %-22s n %3d  counts %s  |rec - oracle| %.2e  surface residual %.2e%s" % (
            label + ("/swap" if swapped else ""), name, s.stop - s.start, "/".join(str(v) for v in hist), worst_ref, worst_inv,
            "  cases with more than one oracle answer %d, answer taken %s, in the oracle's order %d of %d" % (
                unstable, "".join(str(v) if v >= 0 else "?" for v in taken.get(name)), in_order, s.stop - s.start) if tie else ""))
    return bad, taken


# ================================================================================================ cyl_box
def cyl_reference(pc, axis, rad, half, pb, Rb, sb, margin):
    """-> dict(dmin, tm, tp, hit, through, out[7]) at DIGITS digits, rounded to f64 at the end; `gap` = the distance of the hit decision from its threshold and
    `depth_gap` (through only) = the distance between the two smallest face depths."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        F = lambda v: mp.mpf(float(v))
        R = [[F(Rb[3 * r + k]) for k in range(3)] for r in range(3)]
        rel = [F(pc[k]) - F(pb[k]) for k in range(3)]
        c = [sum(rel[r] * R[r][i] for r in range(3)) for i in range(3)]
        u = [sum(F(axis[r]) * R[r][i] for r in range(3)) for i in range(3)]
        s, h = [F(v) for v in sb], F(half)

        def clampv(t):
            x = [c[i] + t * u[i] for i in range(3)]
            return x, [min(max(x[i], -s[i]), s[i]) for i in range(3)]

        def f(t):
            x, q = clampv(t)
            return sum((x[i] - q[i]) ** 2 for i in range(3))

        def g(t):
            x, q = clampv(t)
            return sum(u[i] * (x[i] - q[i]) for i in range(3))

        brk = {-h, h}
        for i in range(3):
            if u[i] != 0:
                for sg in (-1, 1):
                    t = (sg * s[i] - c[i]) / u[i]
                    if -h < t < h:
                        brk.add(t)
        brk = sorted(brk)
        cand = list(brk)
        for a, b in zip(brk[:-1], brk[1:]):      # g is linear on a piece: its root, where it has one inside
            ga, gb = g(a), g(b)
            if ga * gb < 0:
                cand.append(a + (b - a) * (-ga) / (gb - ga))
        dmin = mp.sqrt(min(f(t) for t in cand))
        tol = F(CYL_FLAT)

        # the routine's scan over the sorted knots, in exact arithmetic: a knot with |g| <= tol counts as stationary, a sign change between two knots is
        # interpolated (g is linear in between: the exact root)
        G = [g(t) for t in brk]
        last = len(brk) - 1
        tm, tp = brk[last], brk[0]
        for k in range(last + 1):
            if G[k] >= -tol:
                tm = brk[k] if (k == 0 or G[k] <= tol) else brk[k - 1] + (brk[k] - brk[k - 1]) * (-G[k - 1]) / (G[k] - G[k - 1])
                break
        for k in range(last, -1, -1):
            if G[k] <= tol:
                tp = brk[k] if (k == last or G[k] >= -tol) else brk[k] + (brk[k + 1] - brk[k]) * (-G[k]) / (G[k + 1] - G[k])
                break
        ts = (tm + tp) / 2
        x, q = clampv(ts)
        df = [x[i] - q[i] for i in range(3)]
        ln = mp.sqrt(sum(v * v for v in df))
        through = not ln > F(CYL_THROUGH)
        depth_gap = mp.inf
        if not through:
            nl, dist = [v / ln for v in df], ln - F(rad)
        else:
            dep = [s[i] - abs(x[i]) for i in range(3)]
            bi = min(range(3), key=lambda i: dep[i])
            depth_gap = sorted(dep)[1] - sorted(dep)[0]
            nl = [mp.mpf(0)] * 3
            nl[bi] = mp.mpf(-1 if x[bi] < 0 else 1)
            dist = -dep[bi] - F(rad)
            q[bi] = nl[bi] * s[bi]
        out = [dist] + [F(pb[k]) + sum(R[k][i] * (q[i] + dist * nl[i] / 2) for i in range(3)) for k in range(3)] + [sum(R[k][i] * nl[i] for i in range(3)) for k in range(3)]
        ref_dist = dist if through else dmin - F(rad)
        return dict(dmin=float(dmin), tm=float(tm), tp=float(tp), hit=bool(ref_dist < F(margin)), through=bool(through), out=np.array([float(v) for v in out]),
                    dist=float(ref_dist), gap=float(abs(ref_dist - F(margin))), depth_gap=float(depth_gap), through_gap=float(abs(ln - F(CYL_THROUGH))))


def check_cyl(g, hit, out, label):
    """hit [n], out [n, 7] (pre-filled with NaN).  Returns violations."""
    bad = []
    for name in g.names:
        s = g.rows(name)
        w_d, w_p, w_o, nh, nt = 0.0, 0.0, 0.0, 0, 0
        for i in range(s.start, s.stop):
            tag = "%s[%d]" % (name, i - s.start)
            if bool(hit[i]) != bool(g.ref_hit[i]):
                bad.append("%s: hit %d, reference %d (dist - margin = %.3e)" % (tag, hit[i], g.ref_hit[i], g.ref_dist[i] - g.par[i, 2]))
                continue
            if not hit[i]:
                if not np.isnan(out[i]).all():
                    bad.append("%s: a miss wrote its output" % tag)
                continue
            nh += 1
            nt += int(g.through[i])
            ed, ep = abs(out[i, 0] - g.ref_dist[i]), np.abs(out[i, 1:] - g.ref_out[i, 1:]).max()
            w_d, w_p = max(w_d, ed), max(w_p, ep)
            if not (ed <= ATOL and ep <= ATOL):
                bad.append("%s: dist off by %.2e, pos / normal by %.2e (through %d)" % (tag, ed, ep, g.through[i]))
            if g.orc_hit[i]:
                w_o = max(w_o, np.abs(out[i] - g.orc_out[i]).max())
            if name == "cull":      # gen_phase3 only calls the routine inside this radius: a hit outside it would be lost
                e2, rr = cull_distance2(g.pc[i], g.axis[i], g.par[i, 1], g.pb[i]), np.linalg.norm(g.sb[i]) + g.par[i, 0]
                if not e2 < rr * rr:
                    bad.append("%s: a hit outside the cull radius of gen_phase3" % tag)
        print("%-9s cyl_box %-14s n %3d  hits %3d (through %2d)  |dist - ref| %.2e  |pos, normal - ref| %.2e  |out - oracle| %.2e" % (
            label, name, s.stop - s.start, nh, nt, w_d, w_p, w_o))
    return bad


def cull_distance2(pc, axis, half, pb):
    w = np.asarray(pb, float) - np.asarray(pc, float)
    t = float(np.clip(w @ axis, -half, half))
    e = w - t * np.asarray(axis, float)
    return float(e @ e)


# ================================================================================================ cone
def cone_zone(jar, Dn, Dt, mu, fric, mp):
    """0 top, 1 bottom, 2 middle, at the working precision."""
    N, T = jar[0] * mu, mp.sqrt((jar[1] * fric) ** 2 + (jar[2] * fric) ** 2)
    if N >= mu * T:
        return 0
    return 1 if mu * N + T <= 0 else 2


def cone_reference(jar, Dn, Dt, mu, fric, zone=None):
    """[cost, force3, Hc9] by mpmath differentiation of the zone's cost (zone None: the zone the input lies in), and the zone.  The step of the
    differences is relative to the input (the middle zone's cost is singular on the axis T = 0, an absolute step would cross it near the apex)."""
    import mpmath as mp
    with mp.workdps(4 * DIGITS):
        F = lambda v: mp.mpf(float(v))
        j0, Dn, Dt, mu, fric = [F(v) for v in jar], F(Dn), F(Dt), F(mu), F(fric)
        if Dn == 0:
            return np.zeros(13), -1
        z = cone_zone(j0, Dn, Dt, mu, fric, mp) if zone is None else zone
        Dm = Dn / max(F(1e-15), mu * mu * (1 + mu * mu))

        def cost(a, b, c):
            if z == 0:
                return mp.mpf(0)
            if z == 1:
                return (Dn * a * a + Dt * b * b + Dt * c * c) / 2
            return Dm * (a * mu - mu * mp.sqrt((b * fric) ** 2 + (c * fric) ** 2)) ** 2 / 2

        out = [cost(*j0)]
        if z == 0:
            return np.zeros(13), z
        scale = max(abs(v) for v in j0)
        hstep = scale * mp.mpf(10) ** (-DIGITS)
        for a in range(3):
            o = [0, 0, 0]
            o[a] = 1
            out.append(-mp.diff(cost, tuple(j0), tuple(o), h=hstep))
        for a in range(3):
            for b in range(3):
                o = [0, 0, 0]
                o[a] += 1
                o[b] += 1
                out.append(mp.diff(cost, tuple(j0), tuple(o), h=hstep))
        return np.array([float(v) for v in out]), z


def cone_numpy(jar, Dn, Dt, mu, fric):
    """The yardstick: the same cost's gradient and Hessian written out by hand, plain f64.  r = N - mu T, dr = (mu, -mu fric U / T),
    d2r = -mu fric^2 (I / T - U U' / T^3) on the tangential block."""
    o = np.zeros(13)
    if Dn == 0:
        return o
    j = np.asarray(jar, float)
    with np.errstate(all="ignore"):
        N, U = j[0] * mu, j[1:] * fric
        T = np.sqrt(U @ U)
        if N >= mu * T:
            return o
        if mu * N + T <= 0:
            D = np.array([Dn, Dt, Dt])
            o[0], o[1:4], o[4:] = 0.5 * (D * j * j).sum(), -D * j, np.diag(D).ravel()
            return o
        Dm = Dn / max(1e-15, mu * mu * (1 + mu * mu))
        r = N - mu * T
        dr = np.array([mu, -mu * fric * U[0] / T, -mu * fric * U[1] / T])
        H = np.outer(dr, dr)
        H[1:, 1:] += r * (-mu * fric * fric) * (np.eye(2) / T - np.outer(U, U) / T ** 3)
        o[0], o[1:4], o[4:] = 0.5 * Dm * r * r, -Dm * r * dr, (Dm * H).ravel()
    return o


CONE_PARTS = (("cost", slice(0, 1)), ("force", slice(1, 4)), ("Hc", slice(4, 13)))


def cone_bounds(g):
    """Per family and part (cost, force, Hc): 4 yardsticks, relative to the part's largest reference entry.  [n_fam, 3]"""
    b = np.zeros((len(g.names), 3))
    for fi, name in enumerate(g.names):
        s = g.rows(name)
        for pi, (_, sl) in enumerate(CONE_PARTS):
            if pi == 2 and not g.hess[s].any():
                b[fi, pi] = np.inf
                continue
            rel = 0.0
            for i in range(s.start, s.stop):
                if pi == 2 and not g.hess[i]:
                    continue
                sc = np.abs(g.ref[i, sl]).max()
                e = np.abs(g.yard[i, sl] - g.ref[i, sl]).max()
                if pi == 2 and g.edge[i]:
                    e = min(e, np.abs(g.yard[i, sl] - g.alt[i]).max())
                rel = max(rel, e / sc if sc > 0 else (0.0 if e == 0 else np.inf))
            b[fi, pi] = FACTOR * max(ULP, rel)
    return b


def check_cone(g, out, label):
    """out [n, 13].  Cost and force everywhere; the Hessian where `hess` is set (not in the recorded apex window) - on an `edge` case (a zone boundary at 1e-15
    relative, where f64 rounding decides the zone and the Hessian jumps) the own zone's or the neighbour's.  Returns (violations, worst error / bound,
    {family: finite Hessians} of the families whose Hessian is recorded only)."""
    bad, bounds, worst, fin = [], cone_bounds(g), 0.0, {}
    for fi, name in enumerate(g.names):
        s = g.rows(name)
        ratio = np.zeros(3)
        for i in range(s.start, s.stop):
            tag = "%s[%d]" % (name, i - s.start)
            for pi, (part, sl) in enumerate(CONE_PARTS):
                if pi == 2 and not g.hess[i]:
                    fin[name] = fin.get(name, 0) + int(np.isfinite(out[i, sl]).all())
                    continue
                sc = np.abs(g.ref[i, sl]).max()
                e = np.abs(out[i, sl] - g.ref[i, sl]).max()
                if pi == 2 and g.edge[i]:
                    e = min(e, np.abs(out[i, sl] - g.alt[i]).max())
                if not np.isfinite(out[i, sl]).all():
                    e = np.inf
                lim = bounds[fi, pi] * sc
                if not e <= lim:
                    bad.append("%s: %s off by %.3e > %.3e (zone %d)" % (tag, part, e, lim, g.zone[i]))
                if lim > 0:
                    ratio[pi] = max(ratio[pi], e / lim)
        worst = max(worst, ratio.max())
        print("%-9s cone %-16s n %3d  bound (rel) cost %.1e force %.1e Hc %.1e   worst err / bound %.3f %.3f %.3f%s" % (
            label, name, s.stop - s.start, bounds[fi, 0], bounds[fi, 1], bounds[fi, 2], ratio[0], ratio[1], ratio[2],
            "   finite Hessians %d of %d (recorded)" % (fin[name], s.stop - s.start) if name in fin else ""))
    return bad, worst, fin


# ================================================================================================ ldl
def tri_unpack(a, n):
    A = np.zeros((n, n), dtype=np.asarray(a).dtype)
    A[np.tril_indices(n)] = a
    return A


def ldl_reference(a, b, n):
    """-> (ok, x, pivots): mpmath LDL^T of the stored matrix; ok = every pivot > 1e-300 (the factorisation stops at the first that is not)."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        A = tri_unpack(np.asarray(a, float), n)
        A = A + np.tril(A, -1).T
        L = [[mp.mpf(0)] * n for _ in range(n)]
        d = [mp.mpf(0)] * n
        for j in range(n):
            sj = mp.mpf(float(A[j, j])) - sum(L[j][k] ** 2 * d[k] for k in range(j))
            d[j] = sj
            if not sj > mp.mpf(PIVOT_MIN):
                return False, np.zeros(n), np.array([float(v) for v in d])
            for i in range(j + 1, n):
                L[i][j] = (mp.mpf(float(A[i, j])) - sum(L[i][k] * L[j][k] * d[k] for k in range(j))) / sj
        x = [mp.mpf(float(v)) for v in b]
        for i in range(n):
            x[i] -= sum(L[i][k] * x[k] for k in range(i))
        x = [x[i] / d[i] for i in range(n)]
        for i in range(n - 1, -1, -1):
            x[i] -= sum(L[k][i] * x[k] for k in range(i + 1, n))
        return True, np.array([float(v) for v in x]), np.array([float(v) for v in d])


def ldl_numpy(a, b, n):
    A = tri_unpack(np.asarray(a, float), n)
    A = A + np.tril(A, -1).T
    C = np.linalg.cholesky(A)
    return np.linalg.solve(C.T, np.linalg.solve(C, np.asarray(b, float)))


def ldl_bounds(g):
    b = np.zeros(len(g.names))
    for fi, name in enumerate(g.names):
        s = g.rows(name)
        rel = [np.abs(g.yard[i] - g.x[i]).max() / np.abs(g.x[i]).max() for i in range(s.start, s.stop) if g.ok[i]]
        b[fi] = FACTOR * max([ULP] + rel)
    return b


def check_ldl(g, n, ok, L, d, x, label):
    """Returns (violations, worst error / bound)."""
    bad, bounds, worst = [], ldl_bounds(g), 0.0
    for fi, name in enumerate(g.names):
        s = g.rows(name)
        rx = ra = 0.0
        for i in range(s.start, s.stop):
            tag = "%s[%d]" % (name, i - s.start)
            if bool(ok[i]) != bool(g.ok[i]):
                bad.append("%s: ok %d, reference %d (pivots %s)" % (tag, ok[i], g.ok[i], g.piv[i]))
                continue
            if not (np.isfinite(x[i]).all() and np.isfinite(d[i]).all() and np.isfinite(L[i]).all()):
                bad.append("%s: result not finite" % tag)
                continue
            if not g.ok[i]:
                continue
            ex = np.abs(x[i] - g.x[i]).max() / np.abs(g.x[i]).max()
            Lm = tri_unpack(L[i].astype(np.longdouble), n)
            A = tri_unpack(g.A[i].astype(np.longdouble), n)
            Lm[np.diag_indices(n)] = 1
            rec = (Lm * d[i].astype(np.longdouble)) @ Lm.T
            ea = float(np.abs(np.tril(rec - (A + np.tril(A, -1).T))).max() / np.abs(A).max())
            rx, ra = max(rx, ex / bounds[fi]), max(ra, ea / bounds[fi])
            if not ex <= bounds[fi]:
                bad.append("%s: x off by %.3e (relative) > %.3e" % (tag, ex, bounds[fi]))
            if not ea <= bounds[fi]:
                bad.append("%s: L d L' off A by %.3e (relative) > %.3e" % (tag, ea, bounds[fi]))
        worst = max(worst, rx, ra)
        print("%-9s ldl<%d> %-12s n %3d  bound (rel) %.2e  worst x err / bound %.3f  L d L' - A / bound %.3f  not ok %d" % (
            label, n, name, s.stop - s.start, bounds[fi], rx, ra, int((~g.ok[s].astype(bool)).sum())))
    return bad, worst


# ================================================================================================ cube_integrate
def cube_map_mp(state, acc, h, K):
    import mpmath as mp
    with mp.workdps(DIGITS):
        F = lambda v: mp.mpf(float(v))
        pos, q, vel, a, h = [F(v) for v in state[:3]], [F(v) for v in state[3:7]], [F(v) for v in state[7:]], [F(v) for v in acc], F(h)
        for _ in range(K):
            vel = [vel[k] + h * a[k] for k in range(6)]
            pos = [pos[k] + h * vel[k] for k in range(3)]
            w = vel[3:]
            ang = mp.sqrt(sum(v * v for v in w)) * h
            if ang >= F(1e-15):
                sa, ca = mp.sin(ang / 2), mp.cos(ang / 2)
                dq = [ca] + [v * h / ang * sa for v in w]
                r = [q[0] * dq[0] - q[1] * dq[1] - q[2] * dq[2] - q[3] * dq[3], q[0] * dq[1] + q[1] * dq[0] + q[2] * dq[3] - q[3] * dq[2],
                     q[0] * dq[2] - q[1] * dq[3] + q[2] * dq[0] + q[3] * dq[1], q[0] * dq[3] + q[1] * dq[2] - q[2] * dq[1] + q[3] * dq[0]]
                nn = mp.sqrt(sum(v * v for v in r))
                q = [v / nn for v in r]
        return np.array([float(v) for v in pos + q + vel])


def cube_map_numpy(state, acc, h, K):
    s = np.array(state, float)
    pos, q, vel, a = s[:3].copy(), s[3:7].copy(), s[7:].copy(), np.asarray(acc, float)
    for _ in range(K):
        vel = vel + h * a
        pos = pos + h * vel[:3]
        w = vel[3:]
        ang = np.sqrt(w @ w) * h
        if ang >= 1e-15:
            sa, ca = np.sin(0.5 * ang), np.cos(0.5 * ang)
            dq = np.concatenate([[ca], w * (h / ang) * sa])
            r = np.array([q[0] * dq[0] - q[1:] @ dq[1:], *(q[0] * dq[1:] + dq[0] * q[1:] + np.cross(q[1:], dq[1:]))])
            q = r / np.sqrt(r @ r)
    return np.concatenate([pos, q, vel])


CUBE_PARTS = (("pos", slice(0, 3)), ("quat", slice(3, 7)), ("vel", slice(7, 13)))


def quat_norm_dev(q):
    """| |q| - 1 | in long double; q [..., 4]."""
    q = np.asarray(q, np.longdouble)
    return np.abs(np.sqrt((q * q).sum(axis=-1)) - 1).astype(float)


def check_cube(g, final, norm_dev, label):
    """final [n, 13] after K[i] calls; norm_dev [n] = the largest | |q| - 1 | after any call.  Returns (violations, worst error / bound)."""
    bad, worst = [], 0.0
    for fi, name in enumerate(g.names):
        s = g.rows(name)
        ratio, wn = np.zeros(3), 0.0
        for pi, (part, sl) in enumerate(CUBE_PARTS):
            sc = np.abs(g.ref[s, sl]).max(axis=1)
            rel = np.abs(g.yard[s, sl] - g.ref[s, sl]).max(axis=1) / np.where(sc > 0, sc, 1)
            bound = FACTOR * max(ULP, rel.max())
            for i in range(s.start, s.stop):
                sci = np.abs(g.ref[i, sl]).max()
                e = np.abs(final[i, sl] - g.ref[i, sl]).max()
                if not e <= bound * sci:
                    bad.append("%s[%d]: %s off by %.3e > %.3e" % (name, i - s.start, part, e, bound * sci))
                if sci > 0:
                    ratio[pi] = max(ratio[pi], e / (bound * sci))
        for i in range(s.start, s.stop):
            wn = max(wn, norm_dev[i])
            if not norm_dev[i] <= 4 * ULP:
                bad.append("%s[%d]: | |q| - 1 | reached %.3e > 4 x 2^-52" % (name, i - s.start, norm_dev[i]))
        worst = max(worst, ratio.max())
        print("%-9s cube_integrate %-12s n %3d  K %s  worst err / bound pos %.3f quat %.3f vel %.3f   max | |q| - 1 | %.2e" % (
            label, name, s.stop - s.start, sorted(set(int(k) for k in g.K[s])), ratio[0], ratio[1], ratio[2], wn))
    return bad, worst


# ================================================================================================ push_tan_yaw / quat2mat
def yaw_reference(q):
    """(tan(yaw), R9 of mju_quat2Mat) at DIGITS digits."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        w, x, y, z = [mp.mpf(float(v)) for v in q]
        Nq = w * w + x * x + y * y + z * z
        M = [[mp.mpf(1), 0, 0], [0, mp.mpf(1), 0], [0, 0, mp.mpf(1)]]
        if Nq > mp.mpf(FEPS):      # quat2mat of geometric_transformation.py: identity below FLOAT_EPS
            sc = 2 / Nq
            X, Y, Z = x * sc, y * sc, z * sc
            M = [[1 - (y * Y + z * Z), x * Y - w * Z, x * Z + w * Y], [x * Y + w * Z, 1 - (x * X + z * Z), y * Z - w * X], [x * Z - w * Y, y * Z + w * X, 1 - (x * X + y * Y)]]
        cy = mp.sqrt(M[2][2] ** 2 + M[1][2] ** 2)      # mat2euler
        num, den = (M[0][1], M[0][0]) if cy > 4 * mp.mpf(FEPS) else (-M[1][0], M[1][1])
        yaw = -mp.atan2(num, den)
        if den != 0:         # tan(-atan2(num, den)) = -num / den exactly; through a 40-digit pi, tan(+-pi) would come out as 4e-43 instead of 0
            return float(-num / den), np.array([float(v) for v in [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                                                                       w * w - x * x + y * y - z * z, 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                                                                       w * w - x * x - y * y + z * z]]), float(cy)
        R = [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
             2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]
        return float(mp.tan(yaw)), np.array([float(v) for v in R]), float(cy)


def yaw_numpy(q):
    w, x, y, z = (float(v) for v in q)
    Nq = w * w + x * x + y * y + z * z
    m00, m01, m10, m11, m12, m22 = 1.0, 0.0, 0.0, 1.0, 0.0, 1.0
    if Nq > FEPS:
        sc = 2.0 / Nq
        X, Y, Z = x * sc, y * sc, z * sc
        m00, m01, m10, m11, m12, m22 = 1.0 - (y * Y + z * Z), x * Y - w * Z, x * Y + w * Z, 1.0 - (x * X + z * Z), y * Z - w * X, 1.0 - (x * X + y * Y)
    cy = np.sqrt(m22 * m22 + m12 * m12)
    yaw = -np.arctan2(m01, m00) if cy > 4 * FEPS else -np.arctan2(-m10, m11)
    return float(np.tan(yaw))


def check_yaw(g, tan, R, label):
    """tan [n], R [n, 9].  Returns (violations, worst error / bound)."""
    bad, worst = [], 0.0
    for fi, name in enumerate(g.names):
        s = g.rows(name)
        nz = g.tan[s] != 0      # (a reference of exactly 0 has no relative yardstick: the absolute term is its bound)
        rel = np.abs(g.tan_yard[s] - g.tan[s])[nz] / np.abs(g.tan[s])[nz]
        bt = FACTOR * max([ULP] + list(rel))
        scR = np.abs(g.R[s]).max(axis=1)
        bR = FACTOR * max(ULP, (np.abs(g.R_yard[s] - g.R[s]).max(axis=1) / scR).max())
        rt = rR = 0.0
        for i in range(s.start, s.stop):
            lim = bt * abs(g.tan[i]) + 1e-15
            e = abs(tan[i] - g.tan[i])
            rt = max(rt, e / lim)
            if not e <= lim:
                bad.append("%s[%d]: tan(yaw) %.17g, reference %.17g: off by %.3e > %.3e" % (name, i - s.start, tan[i], g.tan[i], e, lim))
            eR = np.abs(R[i] - g.R[i]).max() / scR[i - s.start]
            rR = max(rR, eR / bR)
            if not eR <= bR:
                bad.append("%s[%d]: quat2mat off by %.3e (relative) > %.3e" % (name, i - s.start, eR, bR))
        worst = max(worst, rt, rR)
        print("%-9s tan_yaw %-14s n %3d  bound (rel) %.2e  worst err / bound %.3f   quat2mat bound %.2e  err / bound %.3f" % (label, name, s.stop - s.start, bt, rt, bR, rR))
    return bad, worst


def check_yaw_f32(g, tan, label, family):
    """The cast the observation applies, (float) tan(yaw), over one family: the reference's f32 value or one of its two neighbours.  Returns violations."""
    bad = []
    s = g.rows(family)
    off, worst = 0, 0.0
    for i in range(s.start, s.stop):
        a, b = np.float32(tan[i]), np.float32(g.tan[i])
        if not (a == b or a == np.nextafter(b, np.float32(np.inf)) or a == np.nextafter(b, np.float32(-np.inf))):
            off += 1
            worst = max(worst, abs(float(a) - float(b)) / float(np.spacing(np.abs(b))))
            bad.append("%s[%d]: the f32 observation %.9g is neither the reference's %.9g nor a neighbour" % (family, i - s.start, a, b))
    print("%-9s tan_yaw f32 %-14s n %3d  beyond a neighbour %d%s" % (label, family, s.stop - s.start, off, "  (worst %.3g f32 ulps of the reference)" % worst if off else ""))
    return bad


# ================================================================================================ the host build of every routine over the stored problems
def host_box(g, swapped=False, cap=8):
    from tests.hostcheck import hostcheck as H
    count, rec = np.zeros(g.n, dtype=np.int32), np.full((g.n, 8, 7), np.nan)
    A, B = (("2", "1") if swapped else ("1", "2"))
    for i in range(g.n):
        count[i], rec[i] = H.box_box_R(getattr(g, "p" + A)[i], getattr(g, "R" + A)[i], getattr(g, "s" + A)[i], getattr(g, "p" + B)[i], getattr(g, "R" + B)[i],
                                       getattr(g, "s" + B)[i], g.margin[i], cap)
    return count, rec


def host_cyl(g):
    from tests.hostcheck import hostcheck as H
    hit, out = np.zeros(g.n, dtype=np.int32), np.full((g.n, 7), np.nan)
    for i in range(g.n):
        hit[i], out[i] = H.cyl_box_axis(g.pc[i], g.axis[i], g.par[i, 0], g.par[i, 1], g.pb[i], g.Rb[i], g.sb[i], g.par[i, 2])
    return hit, out


def host_cone(g, twin):
    from tests.hostcheck import hostcheck as H
    return np.array([H.cone_eval(g.jar[i], *g.par[i], twin=twin) for i in range(g.n)])


def host_ldl(g, n, twin):
    from tests.hostcheck import hostcheck as H
    r = [H.ldl(n, g.A[i], g.b[i], twin) for i in range(g.n)]
    return np.array([v[0] for v in r]), np.array([v[1] for v in r]), np.array([v[2] for v in r]), np.array([v[3] for v in r])


def host_cube(g):
    """(final [n, 13], largest | |q| - 1 | after any call [n]): the chain in one call, and again call by call for the norms (the same bits)."""
    from tests.hostcheck import hostcheck as H
    final, dev = np.zeros((g.n, 13)), np.zeros(g.n)
    for i in range(g.n):
        final[i] = H.cube_integrate(g.state[i], g.acc[i], g.h[i], int(g.K[i]))
        s = g.state[i].copy()
        for _ in range(int(g.K[i])):
            s = H.cube_integrate(s, g.acc[i], g.h[i], 1)
            if np.linalg.norm(s[10:13]) * g.h[i] >= 1e-15:      # (below that the routine leaves the quaternion as it is)
                dev[i] = max(dev[i], quat_norm_dev(s[3:7]))
        assert np.array_equal(s, final[i])
    return final, dev


def host_yaw(g):
    from tests.hostcheck import hostcheck as H
    return np.array([H.tan_yaw(q) for q in g.q]), np.array([H.quat2mat(q) for q in g.q])
