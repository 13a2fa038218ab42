"""ik_solve6 by itself on the host build (tests/hostcheck): which of its three paths every problem of tests/ik_solve6_cases.py takes, and how accurate the
result is against the 40-digit reference - for FAST = false (always Jacobi), FAST = true with a carried vector and FAST = true with a cold one; then the
warm-vector chains, and the controller goldens in the calling form of the kernels (vwarm and trig passed, reset once per launch).
Bounds and their derivation: tests/ik_solve6_cases.py.  The device repeats all of it: tests/test_gpu_ik_solve6.py."""
import numpy as np
import pytest

from tests import ik_solve6_cases as K
from tests.hostcheck import hostcheck as H

LO, HI = K.LO, K.HI


@pytest.fixture(scope="module")
def cases():
    return K.Cases()


def run_host(cases, mode, rows=None):
    """mode 'jacobi': FAST = false; 'warm': FAST = true from K.warm_vectors; 'cold': FAST = true, vwarm[6] = 0.  Returns x, path (1 / 2 / 3) and the vectors left."""
    idx = range(cases.n) if rows is None else rows
    vw = K.warm_vectors(cases)
    if mode == "cold":
        vw[:, 6] = 0.0
    x, path = np.zeros((cases.n, 6)), np.zeros(cases.n, dtype=int)
    for i in idx:
        H.stats(reset=True)
        v = vw[i].copy()
        if mode == "jacobi":
            v[6] = 2.0
        x[i] = H.solve6_warm(cases.A[i], cases.b[i], LO, HI, mode != "jacobi", v)
        eig = H.stats()["eig_calls"]
        if mode == "cold":
            path[i] = 2 if v[6] == 1.0 else (3 if eig else 1)
            assert v[6] in (0.0, 1.0)
        else:
            path[i] = K.path_of(v[6])
        assert eig == (1 if path[i] == 3 else 0), "sentinel %g but %d Jacobi calls" % (v[6], eig)      # the sentinel and the counter tell the same story
        vw[i] = v
    return x, path, vw


@pytest.fixture(scope="module")
def host_runs(cases):
    return {m: run_host(cases, m) for m in ("jacobi", "warm", "cold")}


def test_reference_regenerates(cases):
    """A handful of stored references, evaluated again with mpmath: bit for bit (one problem of every family, first, middle or last)."""
    pytest.importorskip("mpmath")
    for k, name in enumerate(cases.names):
        s = cases.rows(name)
        i = (s.start, (s.start + s.stop) // 2, s.stop - 1)[k % 3]
        x, spec = K.reference(cases.A[i], cases.b[i])
        assert np.array_equal(x, cases.x[i]) and np.array_equal(spec, cases.spec[i]), name
        assert np.abs(K.numpy_solve(cases.A[i], cases.b[i]) - x).max() <= 4 * max(cases.yard[i], K.ULP * cases.xmax[i]), name      # the yardstick is numpy's, to within LAPACK builds


def test_families_are_what_their_names_say(cases):
    """The reference spectrum of every problem prescribes the path its family is named for (no family silently tests another path)."""
    exp = cases.expected()
    want = {"in_range": {1}, "one_0.003": {2}, "one_1e-9": {2}, "two_below": {3}, "one_above_hi": {3}, "trace_over_hi": {3}, "lo_minus_1e-9": {0}, "lo_plus_1e-12": {0},
            "pair_below": {3}, "diagonal": {1, 2, 3}, "diagonal_lo": {3}, "block2": {3}, "chain": {1, 2, 3}}
    for name, w in want.items():
        assert set(exp[cases.rows(name)]) == w, (name, set(exp[cases.rows(name)]))
    for name in ("0.003_and_1.01lo", "b_orthogonal"):
        assert all(K.expected_path(sp) == 2 for sp in cases.spec[cases.rows(name)]), name      # by spectrum path 2; whether the iteration gets there is the 2or3 rule
    for name in ("ik_goldens", "ik_elbow", "ik_wrist"):
        print(name, "paths by spectrum:", {p: int((exp[cases.rows(name)] == p).sum()) for p in (0, 1, 2, 3)})
    assert {1, 2} <= set(exp[cases.rows("ik_goldens")])      # the real matrices cover the plain and the deflated solve


@pytest.mark.parametrize("mode", ["jacobi", "warm", "cold"])
def test_paths_and_accuracy(cases, host_runs, mode):
    x, path, vw = host_runs[mode]
    bad = K.check(cases, x, path, "host/" + mode, assert_path=mode != "jacobi")
    if mode == "jacobi":
        assert (path == 3).all()
    else:
        for name in ("one_0.003", "one_1e-9"):
            assert (path[cases.rows(name)] == 2).all(), name
        for name in ("b_orthogonal", "0.003_and_1.01lo"):
            s = cases.rows(name)
            print("host/%s %s: %d deflated, %d Jacobi" % (mode, name, (path[s] == 2).sum(), (path[s] == 3).sum()))
    assert not bad, "\n".join(bad[:20])


def test_cold_vector_equals_no_vector(cases, host_runs):
    x = np.array([H.solve6(cases.A[i], cases.b[i], LO, HI, True) for i in range(cases.n)])
    assert np.array_equal(x, host_runs["cold"][0])
    xj = np.array([H.solve6(cases.A[i], cases.b[i], LO, HI, False) for i in range(cases.n)])
    assert np.array_equal(xj, host_runs["jacobi"][0])


def test_fast_and_jacobi_agree(cases, host_runs):
    xj, pj, _ = host_runs["jacobi"]
    for mode in ("warm", "cold"):
        xf, pf, _ = host_runs[mode]
        d = np.abs(xf - xj).max(axis=1)
        lim = cases.bound(pf) + cases.bound(pj)
        print("host fast(%s) vs jacobi: worst |dx| / (sum of bounds) %.3f" % (mode, (d / lim).max()))
        assert (d <= lim).all()


def test_warm_chain(cases):
    """The 200-step chain with the vector carried from solve to solve, and the same chain solved cold."""
    s = cases.rows("chain")
    vw = np.zeros(7)
    xs, paths, entered_warm = [], [], []
    H.stats(reset=True)
    for i in range(s.start, s.stop):
        if vw[6] != 0.0:
            vw[6] = 2.0              # a valid vector is any non-zero [6]: 2.0 keeps it valid and shows afterwards whether the call wrote it
        eig0, was = H.stats()["eig_calls"], vw[6]
        x = H.solve6_warm(cases.A[i], cases.b[i], LO, HI, True, vw)
        jac = H.stats()["eig_calls"] - eig0
        assert vw[6] == 0.0 if jac else vw[6] in (was, 1.0)      # a Jacobi call leaves no vector behind; path 1 does not touch it
        p = 3 if jac else (2 if vw[6] == 1.0 else 1)
        xs.append(x); paths.append(p); entered_warm.append(was != 0.0)
    xs, paths, entered_warm = np.array(xs), np.array(paths), np.array(entered_warm)
    warm_used = int(((paths == 2) & entered_warm).sum())
    exp = np.array([K.expected_path(sp) for sp in cases.spec[s]])
    # a step entered with a vector takes exactly the path its spectrum prescribes; one entered cold (the first, and those after a Jacobi call) may fall through
    # from 2 to 3 like the same problem solved on its own (K.FAMILIES, rule "chain")
    ok = (paths == exp) | (exp == 0) | (~entered_warm & (exp == 2) & (paths == 3))
    assert ok.all(), np.nonzero(~ok)
    err, bound = np.abs(xs - cases.x[s]).max(axis=1), cases.base_bound()[s] + cases.deflate_term()[s]
    cold = np.array([H.solve6_warm(cases.A[i], cases.b[i], LO, HI, True, np.zeros(7)) for i in range(s.start, s.stop)])
    print("host chain: paths 1:%d 2:%d 3:%d, %d solves started warm, worst err/bound %.3f, worst |warm - cold| / bound %.3f" % (
        (paths == 1).sum(), (paths == 2).sum(), (paths == 3).sum(), warm_used, (err / bound).max(), (np.abs(xs - cold).max(axis=1) / bound).max()))
    assert (paths == 2).sum() >= 50 and warm_used >= 40 and (paths == 3).sum() >= 4 and (paths == 1).sum() >= 50      # the chain does what it was built for
    assert (err <= bound).all()
    assert (np.abs(xs - cold).max(axis=1) <= bound).all()


@pytest.mark.parametrize("reset", ["per_launch", "never"])
@pytest.mark.parametrize("form", ["vwarm+trig", "vwarm", "trig", "plain"])
@pytest.mark.parametrize("case", K.GOLDEN_CASES)
def test_controller_goldens_in_kernel_form(hostcheck, case, form, reset):
    """test_ik_controller_matches_reference_goldens (test_kernel_math_host.py) through ik_update<true> as the kernels call it: the Avoiding controller wave
    passes vwarm and trig and starts both afresh every n_substeps calls (one launch); the other engines pass vwarm.  Without vwarm the tolerances are that
    test's, 1e-9 on the torque and 1e-13 on ikq; with vwarm the derived path-2 bound of K.golden_bounds (the warm start's accuracy loss, which is kept for its
    speed).  Measured on the host, `limits` with vwarm: torque 1.07e-9, ikq 2.6e-13 (over 1e-9 / 1e-13 from call 45 on; bound at call 99: printed below);
    every other case and form: torque <= 2.7e-11, ikq <= 9.4e-15."""
    g = np.load(K.GOLDEN)
    bt, bq = K.golden_bounds(hostcheck, g, case, "vwarm" in form)
    period = hostcheck.ik_params()["n_substeps"] if reset == "per_launch" else 0
    ikq, ikqd, flags = np.zeros(7), np.zeros(7), 0
    vwarm, trig = (np.zeros(7) if "vwarm" in form else None), (np.zeros(15) if "trig" in form else None)
    et = eq = 0.0
    for k in range(g[case + "__control"].shape[0]):
        if period and k % period == 0:
            if vwarm is not None:
                vwarm[6] = 0.0
            if trig is not None:
                trig[14] = 0.0
        tau, flags = hostcheck.ik_control_form(g[case + "__setpoint"][k], g[case + "__jpos"][k], g[case + "__jvel"][k], ikq, ikqd, flags, True, vwarm, trig)
        et, eq = max(et, np.abs(tau - g[case + "__control"][k]).max()), max(eq, np.abs(ikq - g[case + "__old_q"][k]).max())
        np.testing.assert_allclose(tau, g[case + "__control"][k], rtol=0, atol=bt[k], err_msg="call %d" % k)
        np.testing.assert_allclose(ikq, g[case + "__old_q"][k], rtol=0, atol=bq[k], err_msg="call %d" % k)
    print("host %s %s %s: torque %.2e (bound at the last call %.2e)  ikq %.2e (bound %.2e)" % (case, form, reset, et, bt[-1], eq, bq[-1]))
