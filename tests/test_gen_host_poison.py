"""Read-before-write detector of the generic engine (Pushing, Sorting-2 / 4, Inserting; d3il_amd/csrc/gen_step.h built for the host): with
hc_gen_poison(1) the t area (the device's LDS block, GL_SIZE doubles) and the contact-record area (GG_SIZE doubles) hold NaN before every reset, every
env step and - in the last test - every single sub-step.  A phase that reads a word nobody has written in that step then computes with a NaN.

The comparison is for EQUALITY with the unpoisoned run, not for finiteness: the solvers are full of clamps and selects, and a NaN that enters one can
come out as a finite number (tried while writing this: with the store of a rod contact's regularisation in the joint solver's set-up loop skipped, the
poisoned Sorting episode below stays finite and differs from the clean one from step 73 on).  Every episode asserts its coverage - the rod moved a
cube, and the contact kinds the task is about occurred - so that it cannot pass on a free flight.

This covers the one-lane formulation only; the device's own machinery (parked arm state, set-point exchange, sub-lanes, tree / lone / 64-lane joint
solvers, the blocked record layout) is guarded by the poison library, tests/test_gpu_poison_build.py."""
import os

import numpy as np
import pytest

from d3il_amd.model import blob as blob_mod
from tests.hostcheck.hostcheck import GenHostCheck, _p, lib

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
BAD_FLAGS = 0x1F0000      # solver failure, contact overflow, off table ...
INS_CTX = np.array([[0.42, -0.17, 0.0, np.cos(0.15), 0, 0, np.sin(0.15)], [0.6, -0.08, 0.0, np.cos(-0.25), 0, 0, np.sin(-0.25)],
                    [0.45, 0.02, 0.0, np.cos(0.05), 0, 0, np.sin(0.05)]])
INS_WAY = [(0.45, -0.1), (0.45, 0.12), (0.40, 0.16), (0.40, 0.25)]      # through the blue cube and on into the left gate: the rod ends up on the gate's walls


def _init_qpos():
    return np.load(os.path.join(HERE, "golden", "ref_offline_ik.npz"))["avoiding__traj_last"].copy()


def _context(name):
    if name == "pushing":
        c = np.load(os.path.join(HERE, "golden", "ref_pushing_task.npz"))["test_contexts"][0]
        out = np.zeros(14)
        out[0:2], out[3:7], out[7:9], out[10:14] = c[0:2], c[3:7], c[7:9], c[10:14]
        return out
    if name == "inserting":
        return INS_CTX
    from d3il_amd.envs.sorting import sample_contexts
    nb = 4 if name == "sorting" else 2
    return sample_contexts(60, nb, seed=0)[1].reshape(nb, 7)


def _episode(name, steps, poison, keep=None):
    """One closed-loop scripted episode on the host engine.  Returns the per-step states [steps][rows], the flags, and the coverage record."""
    from d3il_amd.agents import ScriptedPushPolicy
    L = lib()
    hist = np.zeros(80, dtype=np.int64)
    L.hc_gen_island_hist(_p(hist), 1)
    L.hc_gen_poison(poison)
    try:
        h = GenHostCheck(blob_mod.load(name))
        obs = h.reset(_init_qpos(), _context(name))
        pol = None if name == "inserting" else ScriptedPushPolicy("pushing" if name == "pushing" else "sorting", device="cpu")
        des, z = np.array(obs[:2], dtype=float), float(h.s[27])
        states, flags, cov = [], [], dict(rod_cube=0, cube_cube=0, rod_static=0)
        wi = 0
        for t in range(steps):
            if pol is None:      # Inserting: way points (tests/test_inserting_oracle_and_host.py)
                d = np.array(INS_WAY[wi]) - des
                n = np.linalg.norm(d)
                if n < 0.006 and wi < len(INS_WAY) - 1:
                    wi += 1
                des = des + (d / n * min(n, 0.006) if n > 0 else 0)
            else:
                des = des + pol.predict_batch(torch.as_tensor(np.concatenate([des, obs.astype(float)])[None]))[0].numpy()
            obs, _, info = h.step(np.concatenate([des, [z], [0, 1, 0, 0]]), fast=bool(t % 2))[:3]
            states.append(h.s.copy())
            flags.append(info["flags"])
            cubes, nstatic = h.contact_info()
            cov["rod_cube"] += any(c[2] for c in cubes)
            cov["cube_cube"] += any(c[1] for c in cubes)
            cov["rod_static"] += nstatic > 0
            if keep is not None and t == keep[0]:
                keep[1].update(s=h.s.copy(), f=h.f.copy())
        L.hc_gen_island_hist(_p(hist), 0)
        cov["joint_solves"] = int(hist[:36].sum())
        return np.stack(states), np.array(flags), cov
    finally:
        L.hc_gen_poison(0)


def _moved(states, nb):
    """Largest horizontal displacement of a cube between the landing after the reset (step 14) and the end of the episode."""
    a, b = states[14], states[-1]
    return max(float(np.hypot(*(b[42 + 13 * k:44 + 13 * k] - a[42 + 13 * k:44 + 13 * k]))) for k in range(nb))


@pytest.mark.parametrize("name,steps", [("pushing", 70), ("sorting", 100), ("sorting_2", 80), ("inserting", 100)])
def test_generic_engine_reads_nothing_it_has_not_written(name, steps):
    clean, fl0, cov0 = _episode(name, steps, 0)
    dirty, fl1, cov1 = _episode(name, steps, 1)
    nb = {"pushing": 2, "sorting": 4, "sorting_2": 2, "inserting": 3}[name]
    # coverage first: an episode that touches nothing proves nothing
    assert _moved(clean, nb) > 1e-3 and cov0["rod_cube"] > 0, (name, _moved(clean, nb), cov0)
    if name == "sorting":
        assert cov0["joint_solves"] > 0, cov0            # the rod on two cubes: the island the tree solver does not take
    if name == "inserting":
        assert cov0["rod_static"] > 0, cov0              # the rod itself on a wall of the gate
    assert not (fl0 & BAD_FLAGS).any() and not (fl1 & BAD_FLAGS).any(), (hex(int(np.bitwise_or.reduce(fl0))), hex(int(np.bitwise_or.reduce(fl1))))
    assert np.isfinite(dirty).all()
    diff = np.nonzero((clean != dirty).any(axis=1))[0]
    assert diff.size == 0, "%s: the poisoned run differs from step %d on (%d state words)" % (name, diff[0], int((clean != dirty).sum()))
    assert np.array_equal(fl0, fl1) and cov0 == cov1


def test_poison_before_every_single_substep_in_contact():
    """From step 70 of the Sorting episode (the rod on two cubes), sub-steps on their own with the areas poisoned before EACH of them: nothing is carried
    from one sub-step to the next in either area (on the device the parked arm state is; gen_step.h lists the carried words).  The joint PD keeps
    pulling towards the set-point of that step, which lies beyond the cubes: the rod stays pressed against them."""
    kept = {}
    _episode("sorting", 71, 0, keep=(70, kept))
    L = lib()
    runs, covs = [], []
    for poison in (0, 1):
        hist = np.zeros(80, dtype=np.int64)
        L.hc_gen_island_hist(_p(hist), 1)
        L.hc_gen_poison(poison)
        try:
            h = GenHostCheck(blob_mod.load("sorting"))
            h.reset(_init_qpos(), _context("sorting"))
            h.s[:], h.f[:] = kept["s"], kept["f"]
            out, rod = [], 0
            q_des, qd_des = h.s[28:35].copy(), h.s[35:42].copy()      # the controller's joint set-point at the end of step 70, held
            for k in range(200):
                h.substep(*h.control(q_des, qd_des))
                out.append(h.s.copy())
                rod += any(c[2] for c in h.contact_info()[0])
            L.hc_gen_island_hist(_p(hist), 0)
            runs.append(np.stack(out))
            covs.append((rod, int(hist[:36].sum()), int(h.f[0]) & BAD_FLAGS))
        finally:
            L.hc_gen_poison(0)
    assert covs[0][0] > 0 and covs[0][1] > 0 and covs[0][2] == 0, covs      # in contact with the rod, and through the joint solver
    assert np.isfinite(runs[1]).all() and np.array_equal(runs[0], runs[1]) and covs[0] == covs[1]
