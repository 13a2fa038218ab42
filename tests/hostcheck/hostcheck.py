"""ctypes loader for the TEST-ONLY host build of the kernel math (tests/hostcheck/hostcheck.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build(force=False):
    so = os.path.join(_HERE, "libd3il_hostcheck.so")
    srcs = [os.path.join(_HERE, "hostcheck.cpp")] + [os.path.join(_HERE, "..", "..", "d3il_amd", "csrc", f) for f in ("panda_step.h", "panda_consts.h", "rigid_common.h", "gen_step.h", "gen_tree.h", "stack_step.h")]
    srcs.append(os.path.join(_HERE, "..", "..", "include", "d3il_model_blob.h"))
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]])
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.hc_create.restype = C.c_void_p
        _LIB.hc_sizeof_consts.restype = C.c_int
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_sym6(A):
    """The packed lower triangle (21, row by row) of a symmetric 6x6 - ik_solve6's matrix argument."""
    A = np.asarray(A, float)
    return np.ascontiguousarray(A[np.tril_indices(6)])


def solve6(A21, b, lo, hi, fast):
    """ik_solve6<fast> without a warm vector (hc_solve6)."""
    A21, b, x = np.ascontiguousarray(A21, float), np.ascontiguousarray(b, float), np.zeros(6)
    lib().hc_solve6(_p(A21), _p(b), C.c_double(lo), C.c_double(hi), _p(x), int(fast))
    return x


def solve6_warm(A21, b, lo, hi, fast, vwarm=None):
    """ik_solve6<fast> as the kernels call it: vwarm (7 doubles, in/out) or None."""
    A21, b, x = np.ascontiguousarray(A21, float), np.ascontiguousarray(b, float), np.zeros(6)
    lib().hc_solve6_warm(_p(A21), _p(b), C.c_double(lo), C.c_double(hi), _p(x), int(fast), None if vwarm is None else _p(vwarm))
    return x


def stats(reset=False):
    """Host counters: newton_calls, newton_iters, ls_iters, eig_calls, ik_calls, contact_calls."""
    o = (C.c_long * 6)()
    lib().hc_stats(o, int(reset))
    return dict(zip(("newton_calls", "newton_iters", "ls_iters", "eig_calls", "ik_calls", "contact_calls"), o))


class HostCheck:
    def __init__(self, blob):
        self.L = lib()
        err = C.c_char_p()
        self.h = C.c_void_p(self.L.hc_create(C.byref(blob), C.byref(err)))
        if not self.h:
            raise RuntimeError("hc_create: %s" % (err.value.decode() if err.value else "?"))

    def consts(self):
        a, b, m, c = np.zeros(9), np.zeros(1), np.zeros(7), np.zeros((7, 3))
        self.L.hc_get_consts(self.h, _p(a), _p(b), _p(m), _p(c))
        return a, b[0], m, c

    def dynamics(self, q, v):
        q, v = np.ascontiguousarray(q, float), np.ascontiguousarray(v, float)
        M, b, t = np.zeros((9, 9)), np.zeros(9), np.zeros(3)
        self.L.hc_dynamics(self.h, _p(q), _p(v), _p(M), _p(b), _p(t))
        return M, b, t

    def ik_fk(self, q):
        q = np.ascontiguousarray(q, float)
        pos, quat, J = np.zeros(3), np.zeros(4), np.zeros((6, 7))
        self.L.hc_ik_fk(self.h, _p(q), _p(pos), _p(quat), _p(J))
        return pos, quat, J

    def ik_control(self, setpoint, cur_q, cur_v, ikq, ikqd, flags, fast):
        sp, cq, cv = (np.ascontiguousarray(x, float) for x in (setpoint, cur_q, cur_v))
        f = C.c_int(flags)
        tau = np.zeros(7)
        self.L.hc_ik_control(self.h, _p(sp), _p(cq), _p(cv), _p(ikq), _p(ikqd), C.byref(f), int(fast), _p(tau))
        return tau, f.value

    def ik_control_form(self, setpoint, cur_q, cur_v, ikq, ikqd, flags, fast, vwarm=None, trig=None):
        """ik_control in the kernels' calling form: vwarm (7 doubles) / trig (15 doubles) are carried in place, None = not passed."""
        sp, cq, cv = (np.ascontiguousarray(x, float) for x in (setpoint, cur_q, cur_v))
        f = C.c_int(flags)
        tau = np.zeros(7)
        self.L.hc_ik_control_form(self.h, _p(sp), _p(cq), _p(cv), _p(ikq), _p(ikqd), C.byref(f), int(fast), _p(tau),
                                  None if vwarm is None else _p(vwarm), None if trig is None else _p(trig))
        return tau, f.value

    def ik_system(self, setpoint, q):
        """A (packed lower triangle, 21) and right-hand side of the controller's solve at the virtual joint target q."""
        sp, q = np.ascontiguousarray(setpoint, float), np.ascontiguousarray(q, float)
        A, rhs = np.zeros(21), np.zeros(6)
        self.L.hc_ik_system(self.h, _p(sp), _p(q), _p(A), _p(rhs))
        return A, rhs

    def ik_params(self):
        o = np.zeros(35)
        self.L.hc_ik_params(self.h, _p(o))
        return dict(lo=o[0], hi=o[1], J_reg=o[2], lr=o[3], iters=int(o[4]), n_substeps=int(o[5]), q_min=o[6:13].copy(), q_max=o[13:20].copy(),
                    pd_p=o[20:27].copy(), pd_d=o[27:34].copy(), timestep=o[34])

    def physics_substep(self, s, f, tau, ff):
        tau, ff = np.ascontiguousarray(tau, float), np.ascontiguousarray(ff, float)
        self.L.hc_physics_substep(self.h, _p(s), _p(f), _p(tau), _p(ff))

    def env_reset(self, init_qpos):
        init_qpos = np.ascontiguousarray(init_qpos, float)
        s, f, obs = np.zeros(42), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.float32)
        self.L.hc_env_reset(self.h, _p(init_qpos), _p(s), _p(f), _p(obs))
        return s, f, obs

    def env_step(self, s, f, action, fast=True):
        action = np.ascontiguousarray(action, float)
        obs, done = np.zeros(2, dtype=np.float32), np.zeros(1, dtype=np.uint8)
        self.L.hc_env_step(self.h, _p(s), _p(f), _p(action), _p(obs), _p(done), int(fast))
        return obs, bool(done[0])


class GenHostCheck:
    """Host build of the generic engine (d3il_amd/csrc/gen_step.h) running the Sorting task, one environment."""

    def __init__(self, blob):
        self.L = lib()
        self.L.hc_gen_create.restype = C.c_void_p
        err = C.c_char_p()
        self.h = C.c_void_p(self.L.hc_gen_create(C.byref(blob), C.byref(err)))
        if not self.h:
            raise RuntimeError("hc_gen_create: %s" % (err.value.decode() if err.value else "?"))
        nb, ns = C.c_int(0), C.c_int(0)
        st = np.zeros((32, 7))
        self.n = self.L.hc_gen_info(self.h, C.byref(nb), C.byref(ns), _p(st))
        self.nb, self.ns, self.statics = nb.value, ns.value, st[: ns.value].copy()
        ws = np.zeros(8)
        self.ns_core = self.L.hc_gen_workspace(self.h, _p(ws))      # statics [0, ns_core) stand inside the table, the rest are the frame beams around it
        self.inner, self.outer = ws[:4].copy(), ws[4:].copy()      # (lo x, lo y, hi x, hi y) of the beam-free region / of the modelled workspace
        self.n_obs = 2 + 3 * self.nb
        self.s = np.zeros(self.n)
        self.f = np.zeros(2, dtype=np.int32)

    def reset(self, init_qpos, ctx):
        init_qpos, ctx = np.ascontiguousarray(init_qpos, float), np.ascontiguousarray(ctx, float).reshape(7 * self.nb)
        obs = np.zeros(20, dtype=np.float32)
        self.L.hc_gen_reset(self.h, _p(init_qpos), _p(ctx), _p(self.s), _p(self.f), _p(obs))
        return obs[: self.n_obs]

    def step(self, action, fast=True):
        action = np.ascontiguousarray(action, float)
        obs = np.zeros(20, dtype=np.float32)
        done, code = C.c_ubyte(0), C.c_int(0)
        self.L.hc_gen_step(self.h, _p(self.s), _p(self.f), _p(action), _p(obs), C.byref(done), C.byref(code), int(fast))
        fl = int(self.f[0]) & 0xFFFFFFFF
        return obs[: self.n_obs], bool(done.value), dict(mode=code.value, success=bool(fl & (1 << 13)), flags=fl)

    def substep(self, tau, ff):
        tau, ff = np.ascontiguousarray(tau, float), np.ascontiguousarray(ff, float)
        self.L.hc_gen_substep(self.h, _p(self.s), _p(self.f), _p(tau), _p(ff))

    def control(self, q_des, qd_des):
        """Torques of the joint PD + finger PD for the present state (what a sub-step of the env step applies), for substep()."""
        q_des, qd_des = np.ascontiguousarray(q_des, float), np.ascontiguousarray(qd_des, float)
        tau, ff = np.zeros(7), np.zeros(2)
        self.L.hc_gen_control(self.h, _p(self.s), _p(self.f), _p(q_des), _p(qd_des), _p(tau), _p(ff))
        return tau, ff

    def box(self, b):
        o = 42 + 13 * b
        return self.s[o:o + 3], self.s[o + 3:o + 7], self.s[o + 7:o + 13]

    def contact_info(self):
        """The last sub-step's collision result: per cube (contacts, partner-cube mask, rod contact), and the number of rod <-> static box contacts."""
        w = np.zeros(5, dtype=np.int32)
        self.L.hc_gen_contact_info(self.h, _p(w))
        return [(int(x) & 31, (int(x) >> 5) & 15, (int(x) >> 9) & 1) for x in w[: self.nb]], int(w[4])


class PushHostCheck(GenHostCheck):
    """The Pushing task on the host build of the generic engine (gen_step.h, GEN_TASK_PUSHING - the engine the product runs the task on; the round-1 Pushing
    engine is gone), one environment, with the return values of Block_Push_Env.step: state rows 0 .. 88 = arm, cubes, warm start; row 89 info['mean_distance'],
    row 90 the reward; first-visit / mode bits in the flag word."""

    def __init__(self, blob):
        super().__init__(blob)
        assert (self.nb, self.n_obs, self.n) == (2, 8, 91)

    def step(self, action, fast=True):
        obs, done, info = super().step(action, fast)
        fl = info["flags"]
        mode = info["mode"] if info["mode"] < 32768 else info["mode"] - 65536
        return obs, float(self.s[90]), done, dict(mode=mode, success=info["success"], mean_distance=float(self.s[89]), first_visit=(fl & 7) - 1, flags=fl)


class StackHostCheck:
    """Host build of the Stacking engine (d3il_amd/csrc/stack_step.h), one environment."""

    def __init__(self, blob):
        self.L = lib()
        self.L.hc_stack_create.restype = C.c_void_p
        err = C.c_char_p()
        self.h = C.c_void_p(self.L.hc_stack_create(C.byref(blob), C.byref(err)))
        if not self.h:
            raise RuntimeError("hc_stack_create: %s" % (err.value.decode() if err.value else "?"))
        self.n = self.L.hc_stack_state_size()
        self.s = np.zeros(self.n)
        self.f = np.zeros(2, dtype=np.int32)

    def reset(self, init_qpos, ctx):
        init_qpos, ctx = np.ascontiguousarray(init_qpos, float), np.ascontiguousarray(ctx, float).reshape(21)
        obs = np.zeros(12, dtype=np.float32)
        self.L.hc_stack_reset(self.h, _p(init_qpos), _p(ctx), _p(self.s), _p(self.f), _p(obs))
        return obs

    def step(self, action8):
        action8 = np.ascontiguousarray(action8, float).reshape(8)
        obs = np.zeros(12, dtype=np.float32)
        done, md = C.c_ubyte(0), C.c_double(0)
        self.L.hc_stack_step(self.h, _p(self.s), _p(self.f), _p(action8), _p(obs), C.byref(done), C.byref(md))
        fl = int(self.f[0]) & 0xFFFFFFFF
        n = fl & 3
        mode = "".join("rgb"[(fl >> (2 + 2 * i)) & 3] for i in range(n))
        return obs, bool(done.value), dict(mode=mode, success=bool(fl & (1 << 13)), mean_distance=md.value, flags=fl)

    def scratch(self, count):
        """First ``count`` doubles of the solver scratch area (contact records 32 x 36, then the diagnostics of the last sub-step)."""
        out = np.zeros(count)
        self.L.hc_stack_scratch(self.h, _p(out), count)
        return out

    def contacts(self):
        ncon = int(self.scratch(32 * 36 + 4)[32 * 36 + 3])
        out = np.zeros((48, 10))
        n = self.L.hc_stack_contacts(self.h, _p(out))
        return out[:min(n, ncon)]


# ---------------------------------------------------------------- leaf routines of the contact engines by themselves (tests/contact_leaf_cases.py)
def _f(a):
    return np.ascontiguousarray(a, float)


def box_box_R(p1, R1, s1, p2, R2, s2, margin, cap=8):
    """box_box with row-major rotations: (count, rec [8, 7] pre-filled with NaN)."""
    a = [_f(v) for v in (p1, R1, s1, p2, R2, s2)]
    rec = np.full((8, 7), np.nan)
    n = lib().hc_box_box_R(*[_p(v) for v in a], C.c_double(margin), int(cap), _p(rec))
    return n, rec


def cyl_box_axis(pc, axis, rad, half, pb, Rb, sb, margin):
    """cyl_box: (hit, out [7] pre-filled with NaN)."""
    a = [_f(v) for v in (pc, axis, pb, Rb, sb)]
    out = np.full(7, np.nan)
    hit = lib().hc_cyl_box_axis(_p(a[0]), _p(a[1]), C.c_double(rad), C.c_double(half), _p(a[2]), _p(a[3]), _p(a[4]), C.c_double(margin), _p(out))
    return bool(hit), out


def cone_eval(jar, Dn, Dt, mu, fric, twin=False):
    """cone_eval (twin: gt_cone_eval) -> [cost, force3, Hc9]."""
    L = lib()
    L.hc_cone_eval.restype = C.c_double
    jar, o = _f(jar), np.full(13, np.nan)
    f, Hc = np.zeros(3), np.zeros(9)
    o[0] = L.hc_cone_eval(_p(jar), C.c_double(Dn), C.c_double(Dt), C.c_double(mu), C.c_double(fric), _p(f), _p(Hc), int(twin))
    o[1:4], o[4:] = f, Hc
    return o


def ldl(n, A, b, twin=False):
    """ldl_n<n> + ldl_solve_n<n> (twin: gt_*) on the packed lower triangle A -> (ok, L packed, d, x)."""
    A, b = _f(A).copy(), _f(b)
    x, d = np.zeros(n), np.zeros(n)
    ok = lib().hc_ldl(int(n), _p(A), _p(b), _p(x), _p(d), int(twin))
    assert ok >= 0
    return bool(ok), A, d, x


def cube_integrate(state13, acc6, h, K=1):
    s, a = _f(state13).copy(), _f(acc6)
    lib().hc_cube_integrate(_p(s), _p(a), C.c_double(h), int(K))
    return s


def tan_yaw(q):
    L = lib()
    L.hc_tan_yaw.restype = C.c_double
    q = _f(q)
    return L.hc_tan_yaw(_p(q))


def quat2mat(q):
    q, R = _f(q), np.zeros(9)
    lib().hc_quat2mat(_p(q), _p(R))
    return R
