"""The NaN-poison build of ALL kernel families (libd3il_rollout_poison.so, -DD3IL_POISON, built by __graft_entry__.build()): every LDS word of a workgroup
starts as a NaN, so does the generic engine's HBM record area, and what the design does not carry from one sub-step to the next is poisoned again every
sub-step (cooperative engine: stack_kernels.h; generic engine + link-near guard: gen_kernels.h, link_guard.h, the carried words are listed next to the GL_*
layout in gen_step.h; Avoiding split kernel: rollout.hip).  A phase that reads a word its launch has not written then computes with a NaN on every machine -
with the product build the same read returns whatever the memory held before, which differs from machine to machine (round 6: the finger-slide axes of the
rod-robot variants were read by the wrench-form solver although stack_pre_kin writes them for the gripper robot only; some machines ran the Aligning tests
green, others saw NaN states: DESIGN 20.9).

Four checks:
  * the parity files of all six tasks pass in a child process with D3IL_LIB_PATH pointing at the poison library;
  * the guard is live (positive control): in the poison library a resting Sorting scene leaves NaN exactly where no contact record was written, in the
    product library the same area holds no NaN - a build that lost the define, or a fill behind a dead branch, fails here;
  * poison build == product build, bit for bit, on one contact-rich episode per task: the device pass is compiled with -ffinite-math-only and the solvers
    are full of clamps and selects, a NaN that enters one can come out finite, so "no NaN in the output" alone proves nothing;
  * a missing poison library FAILS (it used to skip: a build that silently stopped producing it left the suite green).

What the guard cannot see: private scratch (register spills) cannot be poisoned from source; a poisoned word that is read but whose value is discarded by
a select is, correctly, not reported.  The cooperative engine's guard is unchanged.

Measured wall times of the parity groups on one MI355X (child process each; product library / poison library), and the limit = 3 x the poison time:
    group (child process: python -m pytest -q -m gpu -x <files>)              product   poison (two visits, the larger)   limit
    test_gpu_parity_aligning.py                                                 15.2 s    15.0 s                             45 s
    test_gpu_parity_stacking.py + test_gpu_permutation.py                       53.4 s    55.1 s                            166 s
    test_gpu_parity.py (Avoiding)                                               11.6 s    11.9 s                             36 s
    test_gpu_parity_pushing.py + test_gpu_link_guard.py                         18.3 s    20.3 s                             61 s
    test_gpu_parity_sorting.py                                                  21.6 s    21.7 s                             66 s
    test_gpu_parity_inserting.py                                                21.4 s    22.2 s                             67 s
The guard costs next to nothing at the tests' batch sizes (the fills are a few hundred stores per lane and sub-step next to a contact solve).
The two worker children (tests/poison_ab_worker.py) took 2.6 s (control) and 10.1 s (episodes) on the product library and 26 s for all four children of
both tests together; most of a child is process start (torch import, HIP initialisation: 2 - 3 s here, tens of seconds on a machine that starts cold), so
their limits are a 100 s start-up allowance + 3 x the work, rounded up: 120 s and 180 s.
Whole GPU suite with this file: 172 passed in 537 s (round 6: 385 s; before this file grew: 431 s)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = os.path.join(ROOT, "d3il_amd", "libd3il_rollout_poison.so")
PRODUCT = os.path.join(ROOT, "d3il_amd", "libd3il_rollout.so")
WORKER = os.path.join(ROOT, "tests", "poison_ab_worker.py")

# (files, child time limit in seconds = 3 x the measured time on the poison library)
GROUPS = [
    (("tests/test_gpu_parity_aligning.py",), 45),
    (("tests/test_gpu_parity_stacking.py", "tests/test_gpu_permutation.py"), 166),
    (("tests/test_gpu_parity.py",), 36),
    (("tests/test_gpu_parity_pushing.py", "tests/test_gpu_link_guard.py"), 61),
    (("tests/test_gpu_parity_sorting.py",), 66),
    (("tests/test_gpu_parity_inserting.py",), 67),
]
EPISODES_LIMIT, CONTROL_LIMIT = 180, 120


def _poison_library():
    if os.environ.get("D3IL_LIB_PATH"):
        pytest.skip("already running on a variant library")
    if not os.path.exists(POISON):
        pytest.fail("libd3il_rollout_poison.so not built (python -c 'from d3il_amd import build; build.build_poison()')")
    assert os.path.getmtime(POISON) >= os.path.getmtime(PRODUCT) - 3600, "the poison library is older than the product library: rebuild it"
    return POISON


def _worker(mode, outdir, lib, limit):
    env = dict(os.environ)
    env.pop("D3IL_LIB_PATH", None)
    if lib:
        env["D3IL_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, WORKER, mode, outdir], cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0, "worker (%s, %s) failed:\n%s" % (mode, lib or "product", "\n".join((r.stdout + r.stderr).splitlines()[-15:]))


@pytest.mark.gpu
@pytest.mark.parametrize("files", [g[0] for g in GROUPS])
def test_parity_files_pass_on_the_poison_build(files):
    lib = _poison_library()
    limit = dict(GROUPS)[files]
    env = dict(os.environ, D3IL_LIB_PATH=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"] + list(files), cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0, tail


@pytest.mark.gpu
def test_the_guard_is_live(tmp_path):
    """Positive control.  Sorting, the four cubes of tests/test_sorting_oracle.py::CTX well apart, the set-point held at the start pose for 40 env steps: the
    cubes have landed and rest on the platform (|velocity| < 1e-3 asserted - no free flight), the rod touches nothing.  A resting cube has at most eight
    contact points with the platform, a segment holds GEN_SEG = 24 records.  So in the poison library, per cube segment, record 0 is finite in the fields the
    collision phase stores (0 .. 15: position, frame, distance, kind, a, b; 20, 21: friction, sign - the solver's fields 16 .. 19 stay in registers in the
    lone-cube solver and the arm rows 22 .. 27 belong to rod contacts only) and the LAST record is all NaN; the arm's segment is all NaN (Sorting evaluates
    no rod <-> static pairs).  The product library zero-fills the area once: no NaN anywhere.  The host cannot see the per-segment counts (they live in LDS),
    hence first / last."""
    lib = _poison_library()
    res = {}
    for name, path in (("poison", lib), ("product", None)):      # one GPU process at a time
        out = str(tmp_path / name)
        _worker("control", out, path, CONTROL_LIMIT)
        with open(os.path.join(out, "control.json")) as f:
            res[name] = json.load(f)
        print(name, json.dumps(res[name]))
    from d3il_amd import capi
    p, q = res["poison"], res["product"]
    assert p["build_flags"] & capi.BUILD_POISON and p["build_flags"] & capi.BUILD_SK_POISON, "the poison library was not built with -DD3IL_POISON"
    assert not q["build_flags"] & (capi.BUILD_POISON | capi.BUILD_SK_POISON)
    assert (p["seg"], p["grec"], p["maxnb"], p["gg"]) == (24, 28, 4, 5 * 24 * 28) == (q["seg"], q["grec"], q["maxnb"], q["gg"])
    stored = list(range(16)) + [20, 21]
    for r in (p, q):
        assert r["state_finite"] and not (r["flags_or"] & 0x1F0000)
        assert r["max_cube_speed"] < 1e-3 and r["cube_xy_drift"] < 5e-3, "the cubes are meant to rest where they were put"
    for e in p["envs"]:
        for b in range(4):
            assert all(e["finite_mask_record0"][b][k] for k in stored), (b, e["finite_mask_record0"][b])
            assert 1 <= e["finite_records"][b] <= 8, e["finite_records"]                   # a resting cube: at most eight contact points
            assert e["last_record_nan"][b] == p["grec"], e["last_record_nan"]
        assert e["arm_segment_nan"] == p["seg"] * p["grec"] and e["finite_records"][4] == 0
    for e in q["envs"]:
        assert e["nan_total"] == 0


@pytest.mark.gpu
def test_poison_build_equals_product_build_bit_for_bit(tmp_path):
    """One deterministic episode per task of the families this guard was extended to (tests/poison_ab_worker.py: the episodes of test_gpu_permutation.py at
    256 environments; Avoiding with the serving wave and in the two-wave form), once per library, states and flags of every step compared with
    np.array_equal.  A poisoned word that reaches a result makes the runs differ even where a clamp or select turned the NaN into a finite number."""
    lib = _poison_library()
    dirs = {}
    for name, path in (("poison", lib), ("product", None)):
        dirs[name] = str(tmp_path / name)
        _worker("episodes", dirs[name], path, EPISODES_LIMIT)
    from d3il_amd import capi
    flags = {k: json.load(open(os.path.join(d, "build.json")))["build_flags"] for k, d in dirs.items()}
    assert flags["poison"] & capi.BUILD_POISON and not flags["product"] & capi.BUILD_POISON
    for task in ("avoiding", "avoiding_two_wave", "pushing", "sorting", "inserting"):
        a, b = np.load(os.path.join(dirs["product"], task + ".npy")), np.load(os.path.join(dirs["poison"], task + ".npy"))
        n = a.shape[2]
        fl = a[:, -1].astype(np.int64)
        # coverage, on the product run: the episode has to reach the contacts (as in tests/test_gpu_permutation.py)
        assert np.isfinite(a).all() and not (fl & (1 << 16)).any(), task
        if task.startswith("avoiding"):
            assert ((fl[-1] & (1 << 14)) | (fl[-1] & (1 << 12))).any(), "no environment reached an obstacle"
        else:
            moved = int((np.abs(a[-1, 42:44] - a[0, 42:44]).max(axis=0) > 1e-3).sum())
            assert moved > n // 2, "%s: the scripted policy has to reach the cubes (%d of %d moved)" % (task, moved, n)
        assert a.shape == b.shape
        if not np.array_equal(a, b):
            t = int(np.nonzero((a != b).any(axis=(1, 2)))[0][0])
            envs = np.nonzero((a[t] != b[t]).any(axis=0))[0]
            rows = np.nonzero((a[t] != b[t]).any(axis=1))[0]
            pytest.fail("%s: the poison build differs from the product build from env step %d on: %d environments (first %s), state rows %s, NaN in the poison run: %s"
                        % (task, t, envs.size, envs[:6].tolist(), rows[:12].tolist(), bool(np.isnan(b[t]).any())))
