"""Problems and reference values of the clipped-eigenvalue 6x6 solve (ik_solve6, d3il_amd/csrc/panda_step.h), shared by the host suite
(tests/test_ik_solve6_host.py) and the device suite (tests/test_gpu_ik_solve6.py).

The operation:  x = sum_i (v_i . b) / clip(l_i, lo, hi) v_i  over the eigenpairs (l_i, v_i) of the symmetric A.

tests/golden/ik_solve6_cases.npz (written by tests/golden/gen_ik_solve6_goldens.py) holds, per problem: A (packed lower triangle, as the kernels take it), b,
the reference x and spectrum (mpmath `eigsy` at 40 digits on the f64 matrix AS STORED, rounded to f64 at the end), and the error of a plain numpy-f64 `eigh`
evaluation of the same formula against that reference - the yardstick.

The three paths of the kernel, and what a problem's reference spectrum says it must take (FAST = true; FAST = false is always path 3):
  1  plain LDL^T solve          no eigenvalue below lo, trace < hi
  2  one deflated eigenpair     exactly one eigenvalue below lo, trace < hi
  3  cyclic Jacobi              two or more below lo, or trace >= hi
The kernel reports its path in vwarm[6] when that is preset to 2.0: 2.0 untouched = path 1, 1.0 = deflation accepted, 0.0 = Jacobi.

Bounds.  A family's yardstick is the worst relative error |x_numpy - x_ref|_max / |x_ref|_max of its problems, floored at 2^-52: where numpy is exact (a
diagonal matrix) no f64 routine that rounds more than once can promise less than one unit of the last place.  Paths 1 and 3 are held to 4 yardsticks, the
project's usual factor.  Path 2 gets one added term that follows from the kernel's own acceptance rule, eigen-residual <= 1e-14 trace(A): the accepted vector is
off by at most d = 1e-14 tr / gap (gap: distance from l_1 to the rest of the spectrum), and x = A^-1 (b - (v.b) v) + (v.b) / lo v then moves by at most
|d| |b| (1 / l_1 + 1 / lo); with the same factor 4:   4 (1e-14 tr / gap) |b|_2 (1 / l_1 + 1 / lo).
"""
import os

import numpy as np

LO, HI = 0.01, 100.0      # the blobs' ik_min_sv / ik_max_sv
NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ik_solve6_cases.npz")
DIGITS = 40
ACCEPT = 1e-14            # ik_deflate's acceptance bound on the eigen-residual, relative to trace(A)
FACTOR = 4.0
ULP = 2.0 ** -52

# family -> what is asserted about the path with FAST = true: "spectrum" (the rule above), "2" (every problem deflates), "2or3", "3", "any" (boundary: either side),
# "chain": the rule above, but a problem whose spectrum says 2 may fall through to 3 when solved on its own - the chain's right-hand side sweeps through
# orthogonality to the clipped eigenvector (t = 35) and its last steps have the second eigenvalue at 1.02 lo, the two conditions of the "2or3" families; the
# carried-vector test (test_warm_chain) asserts the chain's paths exactly
FAMILIES = {
    "in_range": "spectrum", "one_0.003": "2", "one_1e-9": "2", "two_below": "spectrum", "one_above_hi": "spectrum", "trace_over_hi": "spectrum",
    "lo_minus_1e-9": "any", "0.003_and_1.01lo": "2or3", "lo_plus_1e-12": "any", "pair_below": "spectrum", "b_orthogonal": "2or3",
    "diagonal": "spectrum", "diagonal_lo": "3", "block2": "spectrum",
    "ik_goldens": "spectrum", "ik_elbow": "spectrum", "ik_wrist": "spectrum",
    "chain": "chain",
}
TRI = np.tril_indices(6)


def unpack_sym6(A21):
    A = np.zeros((6, 6))
    A[TRI] = A21
    return A + np.tril(A, -1).T


def reference(A21, b, lo=LO, hi=HI):
    """(x, spectrum) of one problem at DIGITS digits, rounded to f64: the generator's evaluation, and what test_reference_regenerates repeats."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        A = unpack_sym6(np.asarray(A21, float))
        M = mp.matrix(6, 6)
        for i in range(6):
            for j in range(6):
                M[i, j] = mp.mpf(float(A[i, j]))
        E, Q = mp.eigsy(M)
        x = [mp.mpf(0)] * 6
        for i in range(6):
            vb = sum(Q[k, i] * mp.mpf(float(b[k])) for k in range(6))
            li = min(max(E[i], mp.mpf(lo)), mp.mpf(hi))
            for k in range(6):
                x[k] += vb / li * Q[k, i]
        return np.array([float(v) for v in x]), np.sort(np.array([float(E[i]) for i in range(6)]))


def numpy_solve(A21, b, lo=LO, hi=HI):
    """The yardstick: the same formula through numpy's f64 eigh."""
    w, V = np.linalg.eigh(unpack_sym6(np.asarray(A21, float)))
    return V @ ((V.T @ np.asarray(b, float)) / np.clip(w, lo, hi))


def expected_path(spec, lo=LO, hi=HI):
    """Path the reference spectrum prescribes for FAST = true; 0 when an eigenvalue (or the trace) is within 1e-8 relative of its threshold - either side is right."""
    spec = np.asarray(spec)
    if np.any(np.abs(spec - lo) <= 1e-8 * lo) or abs(spec.sum() - hi) <= 1e-8 * hi:
        return 0
    below = int((spec < lo).sum())
    if below >= 2 or spec.sum() >= hi:
        return 3
    return 2 if below == 1 else 1


class Cases:
    def __init__(self, path=NPZ):
        g = np.load(path)
        self.names = [str(s) for s in g["names"]]
        self.start = g["start"]                      # problems of family i: start[i] .. start[i + 1]
        self.A, self.b, self.x, self.spec, self.yard = g["A"], g["b"], g["x_ref"], g["spec"], g["yard"]
        self.n = len(self.A)
        self.fam = np.repeat(np.arange(len(self.names)), np.diff(self.start))
        self.xmax = np.abs(self.x).max(axis=1)
        self.fam_yard = np.array([max(ULP, (self.yard[s] / self.xmax[s]).max()) for s in (self.rows(n) for n in self.names)])

    def rows(self, name):
        i = self.names.index(name)
        return slice(int(self.start[i]), int(self.start[i + 1]))

    def base_bound(self):
        """4 yardsticks of the problem's family, absolute, per problem."""
        return FACTOR * self.fam_yard[self.fam] * self.xmax

    def deflate_term(self):
        """The added term of path 2, per problem (what it would be if the problem deflated its smallest eigenpair)."""
        l1, gap = self.spec[:, 0], self.spec[:, 1] - self.spec[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = FACTOR * (ACCEPT * self.spec.sum(axis=1) / gap) * np.linalg.norm(self.b, axis=1) * (1.0 / np.abs(l1) + 1.0 / LO)
        return np.where(np.isfinite(t), t, np.inf)

    def bound(self, path):
        """Per-problem bound for the path each problem took (array of 1 / 2 / 3)."""
        return self.base_bound() + np.where(np.asarray(path) == 2, self.deflate_term(), 0.0)

    def expected(self):
        """Per problem: 1 / 2 / 3 asserted, 0 = either of 2 and 3 or a boundary case, with the family's rule applied."""
        out = np.zeros(self.n, dtype=int)
        for name in self.names:
            rule, s = FAMILIES[name], self.rows(name)
            if rule in ("spectrum", "chain"):
                out[s] = [expected_path(sp) for sp in self.spec[s]]
            elif rule in ("2", "3"):
                out[s] = int(rule)
        return out


def warm_vectors(cases, seed=7, lag=1e-3):
    """A plausible carried vector per problem: numpy's eigenvector of the smallest eigenvalue turned by `lag` (the previous solve's vector of a matrix that has
    moved a little), unit length; [6] = 2.0, the path sentinel."""
    rng = np.random.default_rng(seed)
    vw = np.zeros((cases.n, 7))
    for i in range(cases.n):
        v = np.linalg.eigh(unpack_sym6(cases.A[i]))[1][:, 0] + lag * rng.standard_normal(6)
        vw[i, :6] = v / np.linalg.norm(v)
    vw[:, 6] = 2.0
    return vw


def check(cases, x, path, label, assert_path=True):
    """Prints one line per family (kernel error, yardstick, ratio, path counts) and returns the list of violations (empty = pass).
    path: 1 / 2 / 3 per problem as the kernel reported it; where only deflation can be told apart (cold vector on the device) 0 = path 1 or 3."""
    x, path = np.asarray(x), np.asarray(path)
    err = np.abs(x - cases.x).max(axis=1)
    bound, exp = cases.bound(path), cases.expected()
    bad = []
    for fi, name in enumerate(cases.names):
        s = cases.rows(name)
        rel = (err[s] / cases.xmax[s]).max()
        cnt = [int((path[s] == p).sum()) for p in (1, 2, 3, 0)]
        print("%-9s %-17s err %.2e  yardstick %.2e  ratio %6.2f  worst err/bound %.3f  paths 1:%d 2:%d 3:%d%s" % (
            label, name, rel, cases.fam_yard[fi], rel / cases.fam_yard[fi], (err[s] / bound[s]).max(), cnt[0], cnt[1], cnt[2], " 1|3:%d" % cnt[3] if cnt[3] else ""))
        for i in range(s.start, s.stop):
            if not err[i] <= bound[i]:
                bad.append("%s[%d]: |x - x_ref| %.3e > bound %.3e (path %d)" % (name, i - s.start, err[i], bound[i], path[i]))
            if assert_path:
                ok = True
                if FAMILIES[name] == "2or3":
                    ok = path[i] in (2, 3, 0)      # (0: not deflated, seen from a cold vector on the device - the carried-vector mode tells 3 from 1)
                elif exp[i] != 0:
                    ok = path[i] == exp[i] or (path[i] == 0 and exp[i] in (1, 3)) or (FAMILIES[name] == "chain" and exp[i] == 2 and path[i] in (3, 0))
                if not ok:
                    bad.append("%s[%d]: path %d, expected %s (spectrum %s)" % (name, i - s.start, path[i], exp[i] or FAMILIES[name], cases.spec[i]))
    return bad


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ik_controller.npz")
GOLDEN_CASES = ("walk", "far", "limits", "unnorm")
TOL_TAU, TOL_IKQ = 1e-9, 1e-13      # test_ik_controller_matches_reference_goldens (tests/test_kernel_math_host.py)


def golden_bounds(hc, g, case, with_vwarm):
    """Per-call bounds (torque, ikq) of a controller golden replayed through ik_update<true>.

    Without a carried vector they are the tolerances of test_ik_controller_matches_reference_goldens, 1e-9 and 1e-13.  With one (the kernels' calling form) a
    deflated solve is accepted as soon as its eigen-residual is under 1e-14 trace(A), and one Rayleigh-quotient step from the previous vector lands just under
    that, call after call with the same sign, where a cold start ends at round-off (profiles/ik_solve6/README.md; a stopping rule that removes it costs 2 % of
    the Avoiding headline and was not kept, DESIGN section on the IK solve).  So that form gets the path-2 term of the solve, carried through the update:
      one iteration moves ikq by ik_lr (qn + J^T x), the norm clip only shrinks it, so an error dx of the solve moves ikq by at most ik_lr |J|_2 |dx|_2, and
      |dx|_2 <= D = 4 (1e-14 tr / gap) |b|_2 (1 / l_1 + 1 / lo) whenever A has exactly one eigenvalue under lo and trace < hi (else D = 0);
      ikq after call k:   1e-13 + sum_{j <= k} ik_iters ik_lr |J_j|_2 D_j = 1e-13 + E_k,  system j taken at the golden's ikq before call j (the ik_iters
      iterations of a call move the joints by at most ik_iters * 3 * ik_lr = 0.009 rad; the factor 4 in D covers the change of tr, gap and b over that);
      torque = pd_p (ikq - q) + pd_d ((ikq_k - ikq_{k-1}) / timestep - v):   1e-9 + max pd_p E_k + max pd_d (E_k - E_{k-1}) / timestep."""
    n = g[case + "__control"].shape[0]
    bt, bq = np.full(n, TOL_TAU), np.full(n, TOL_IKQ)
    if not with_vwarm:
        return bt, bq
    P = hc.ik_params()
    E = 0.0
    for k in range(n):
        q = g[case + "__old_q"][k - 1] if k else g[case + "__jpos"][0]
        A21, rhs = hc.ik_system(g[case + "__setpoint"][k], q)
        w = np.linalg.eigvalsh(unpack_sym6(A21))
        dE = 0.0
        if (w < P["lo"]).sum() == 1 and w.sum() < P["hi"]:
            D = FACTOR * (ACCEPT * w.sum() / (w[1] - w[0])) * np.linalg.norm(rhs) * (1.0 / w[0] + 1.0 / P["lo"])
            dE = P["iters"] * P["lr"] * np.linalg.norm(hc.ik_fk(q)[2], 2) * D
        E += dE
        bq[k] += E
        bt[k] += P["pd_p"].max() * E + P["pd_d"].max() * dE / P["timestep"]
    return bt, bq


def path_of(sentinel):
    """vwarm[6] after a call that was entered with 2.0 -> 1 / 2 / 3."""
    return {2.0: 1, 1.0: 2, 0.0: 3}[float(sentinel)]
