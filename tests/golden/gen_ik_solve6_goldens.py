"""Writes tests/golden/ik_solve6_cases.npz: the problems of tests/ik_solve6_cases.py (built from seeds) with their 40-digit reference values.

    python tests/golden/gen_ik_solve6_goldens.py        (needs mpmath and the host check library; about a minute)

Families (64 problems each, the chain 200): see FAMILIES in tests/ik_solve6_cases.py.  The matrices are stored as built; the reference is evaluated on the stored
f64 matrix, so nothing depends on how the generating machine's LAPACK or libm rounds.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import ik_solve6_cases as K      # noqa: E402

LO, HI, N = K.LO, K.HI, 64


def orth(rng):
    q, r = np.linalg.qr(rng.standard_normal((6, 6)))
    return q * np.sign(np.diag(r))


def sym(Q, e):
    A = (Q * e) @ Q.T
    return 0.5 * (A + A.T)


def logu(rng, a, b, n):
    return np.exp(rng.uniform(np.log(a), np.log(b), n))


def spectral(seed, spectrum, b_orth=False, b_generic=False):
    """N problems A = Q diag(e) Q^T, Q random orthogonal, e = spectrum(rng), b standard normal.
    b_generic (the families in which EVERY problem must deflate): b's component along the clipped eigenvector is at least 0.5.  A cold solve starts from two
    inverse iterations on b, which raise that component by (l_2 / l_1)^2 >= (0.02 / 0.003)^2 = 44 over every other; with 0.5 of a |b| of about 2.4 the start
    vector is within tan = 0.1 of the eigenvector, and the cubically convergent Rayleigh-quotient steps reach round-off in three of the four the kernel allows.
    A standard normal b falls under 0.02 |b| once in 60 problems and then converges to the NEXT eigenvector: that is the b_orthogonal family's subject."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        e = np.asarray(spectrum(rng), float)
        Q, b = orth(rng), rng.standard_normal(6)
        if b_orth:      # remove the clipped direction from b (to round-off: the component left is ~1e-16 |b|)
            v = Q[:, int(np.argmin(e))]
            b = b - (v @ b) * v
        if b_generic:
            v = Q[:, int(np.argmin(e))]
            c = v @ b
            b = b + (np.copysign(max(abs(c), 0.5), c) - c) * v
        out.append((sym(Q, e), b))
    return out


def rest(rng, n):
    return logu(rng, 0.02, 10.0, n)


def random_families():
    f = {}
    f["in_range"] = spectral(101, lambda r: rest(r, 6))
    f["one_0.003"] = spectral(102, lambda r: np.r_[0.003, rest(r, 5)], b_generic=True)
    f["one_1e-9"] = spectral(103, lambda r: np.r_[1e-9, rest(r, 5)], b_generic=True)
    f["two_below"] = spectral(104, lambda r: np.r_[logu(r, 1e-4, 0.008, 2), rest(r, 4)])
    f["one_above_hi"] = spectral(105, lambda r: np.r_[logu(r, 120.0, 1000.0, 1), rest(r, 5)])
    f["trace_over_hi"] = spectral(106, lambda r: np.r_[r.uniform(40.0, 60.0, 3), rest(r, 3)])
    f["lo_minus_1e-9"] = spectral(107, lambda r: np.r_[LO * (1 - 1e-9), rest(r, 5)])
    f["0.003_and_1.01lo"] = spectral(108, lambda r: np.r_[0.003, 1.01 * LO, rest(r, 4)])
    f["lo_plus_1e-12"] = spectral(109, lambda r: np.r_[LO * (1 + 1e-12), rest(r, 5)])
    f["pair_below"] = spectral(110, lambda r: np.r_[0.005, 0.005 * (1 + 1e-9), rest(r, 4)])
    f["b_orthogonal"] = spectral(111, lambda r: np.r_[0.003, rest(r, 5)], b_orth=True)
    return f


def structured_families():
    f = {}
    rng = np.random.default_rng(201)
    # diagonal: every Jacobi rotation is skipped (apq == 0); the entries span all three paths
    f["diagonal"] = [(np.diag(logu(rng, 1e-3, 30.0, 6)), rng.standard_normal(6)) for _ in range(N)]
    # one entry exactly lo: the shifted pivot is exactly 0, ldl6 reports failure, the 1e-30 guard and Jacobi run
    out = []
    for _ in range(N):
        d = logu(rng, 0.02, 10.0, 6)
        d[rng.integers(6)] = LO
        out.append((np.diag(d), rng.standard_normal(6)))
    f["diagonal_lo"] = out
    out = []
    for _ in range(N):
        p, q = sorted(rng.choice(6, 2, replace=False))
        A = np.zeros((6, 6))
        a, d, c = logu(rng, 0.02, 10.0, 1)[0], logu(rng, 0.02, 10.0, 1)[0], rng.uniform(-0.9, 0.9)
        A[p, p], A[q, q] = a, d
        A[p, q] = A[q, p] = c * np.sqrt(a * d)
        out.append((A, rng.standard_normal(6)))
    f["block2"] = out
    return f


def ik_families():
    """A = J J^T + ik_J_reg I and the controller's right-hand side at real configurations (tests/hostcheck: hc_ik_system)."""
    from d3il_amd.model import blob
    from tests.hostcheck.hostcheck import HostCheck
    hc = HostCheck(blob.load("avoiding"))
    P = hc.ik_params()
    assert (P["lo"], P["hi"]) == (LO, HI)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_ik_controller.npz"))
    f = {}
    out = []
    for case in ("limits", "far"):
        n = g[case + "__old_q"].shape[0]
        for k in np.linspace(0, n - 1, N // 2).round().astype(int):
            out.append(hc.ik_system(g[case + "__setpoint"][k], g[case + "__old_q"][k]))
    f["ik_goldens"] = out
    sp, q0 = g["limits__setpoint"][0], np.clip(g["far__old_q"][-1], P["q_min"], P["q_max"])
    for name, j, end in (("ik_elbow", 3, P["q_max"][3]), ("ik_wrist", 5, 0.0)):
        out = []
        for t in np.linspace(0.0, 1.0, N):
            q = q0.copy()
            q[j] = np.clip(q0[j] + (end - q0[j]) * (1.0 - (1.0 - t) ** 3), P["q_min"][j], P["q_max"][j])      # steps shrink towards the singular end
            out.append(hc.ik_system(sp, q))
        f[name] = out
    return {k: [(K.unpack_sym6(A), b) for A, b in v] for k, v in f.items()}


def givens(i, j, a):
    G = np.eye(6)
    G[i, i] = G[j, j] = np.cos(a)
    G[i, j], G[j, i] = -np.sin(a), np.sin(a)
    return G


def chain_family(T=200):
    """A_t = Q_t diag(e_t) Q_t^T with a slowly turning Q_t; the smallest eigenvalue crosses lo eight times, the second comes below lo
    at the end (t = 189 .. 196 have two below: Jacobi; from t = 197 the one below belongs to another eigenvector than the carried one)."""
    rng = np.random.default_rng(301)
    Q0, b0, b1 = orth(rng), rng.standard_normal(6), rng.standard_normal(6)
    out = []
    for t in range(T):
        Q = Q0 @ givens(0, 1, 0.003 * t) @ givens(2, 3, 0.002 * t) @ givens(4, 5, 0.0025 * t) @ givens(0, 5, 0.0015 * t)
        e1 = LO * (1.0 + 0.5 * np.sin(2 * np.pi * (t + 3.3) / 50.0))
        e2 = 0.05 if t < 170 else max(0.006, 0.05 + (0.006 - 0.05) * (t - 170) / 20.0)      # below lo from t = 189; e1 comes back over lo at t = 197
        out.append((sym(Q, np.array([e1, e2, 0.5, 1.0, 2.0, 5.0])), b0 + 0.01 * t * b1))
    return out


def build_all():
    fams = {}
    fams.update(random_families())
    fams.update(structured_families())
    fams.update(ik_families())
    fams["chain"] = chain_family()
    assert list(fams) == list(K.FAMILIES)
    return fams


def main():
    fams = build_all()
    names, start, A, b, x, spec, yard = [], [0], [], [], [], [], []
    for name, probs in fams.items():
        names.append(name)
        for Af, bf in probs:
            A21 = np.ascontiguousarray(Af[K.TRI])
            xr, sp = K.reference(A21, bf)
            A.append(A21); b.append(bf); x.append(xr); spec.append(sp)
            yard.append(np.abs(K.numpy_solve(A21, bf) - xr).max())
        start.append(len(A))
        s = slice(start[-2], start[-1])
        xm = np.abs(np.array(x[s])).max(axis=1)
        print("%-18s n %3d  yardstick (worst relative numpy error) %.2e" % (name, start[-1] - start[-2], (np.array(yard[s]) / xm).max()))
    np.savez_compressed(K.NPZ, names=np.array(names), start=np.array(start), A=np.array(A), b=np.array(b), x_ref=np.array(x), spec=np.array(spec), yard=np.array(yard))
    print("wrote", K.NPZ, os.path.getsize(K.NPZ), "bytes")


if __name__ == "__main__":
    main()
