"""ctypes loader for the TEST-ONLY device build of the kernels' leaf math (tests/devcheck/devcheck.hip), built like tests/hostcheck but with hipcc and the
product's flags (d3il_amd.build.HIPCC_FLAGS), so that the device-only arithmetic (v_rcp_f64 / v_rsq_f64 + Newton, finite-math, no signed zeros, FMA
contraction) is the product's.  Never loaded by d3il_amd/.  Every call takes torch tensors on the GPU and runs on torch's current stream."""
import ctypes as C
import glob
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = None
EINVAL = -1


def build(force=False):
    from d3il_amd import build as b
    so = os.path.join(_HERE, "libd3il_devcheck.so")
    src = os.path.join(_HERE, "devcheck.hip")
    deps = [src] + glob.glob(os.path.join(_ROOT, "d3il_amd", "csrc", "*.h")) + [os.path.join(_ROOT, "d3il_amd", "csrc", "gen", "avoiding_consts.inc"),
                                                                                  os.path.join(_ROOT, "include", "d3il_model_blob.h")]
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in deps):
        b.check_compiler()
        subprocess.check_call([b.hipcc()] + b.HIPCC_FLAGS + ["-o", so, src], cwd=_ROOT)
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        V, D, I = C.c_void_p, C.c_double, C.c_int
        _LIB.dc_solve6.argtypes = [V, V, D, D, V, V, I, I, V]
        _LIB.dc_solve6_chain.argtypes = [V, V, D, D, V, V, I, I, I, I, V]
        _LIB.dc_scalar.argtypes = [V, V, V, I, V]
        _LIB.dc_trig_chain.argtypes = [V, V, V, I, I, V]
        _LIB.dc_ik_update.argtypes = [V, V, V, V, V, V, I, I, I, I, I, V]
        _LIB.dc_box_box.argtypes = [V, V, V, V, V, V, V, I, V, V, I, V]
        _LIB.dc_cyl_box.argtypes = [V, V, V, V, V, V, V, V, I, V]
        _LIB.dc_cone_eval.argtypes = [V, V, V, I, V]
        _LIB.dc_ldl.argtypes = [I, I, V, V, V, V, V, V, I, V]
        _LIB.dc_cube_chain.argtypes = [V, V, V, I, V, I, V]
        _LIB.dc_tan_yaw.argtypes = [V, V, I, V]
        _LIB.dc_quat2mat.argtypes = [V, V, I, V]
    return _LIB


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def solve6(A, b, lo, hi, x, vwarm, fast, n):
    """A [n, 21], b [n, 6] -> x [n, 6]; vwarm [n, 7] in/out or None.  Returns the entry's code (0 = launched)."""
    return lib().dc_solve6(_p(A), _p(b), lo, hi, _p(x), _p(vwarm), int(fast), int(n), _stream())


def solve6_chain(A, b, lo, hi, x, sent, fast, mark, T, n):
    """A [T, n, 21], b [T, n, 6] -> x [T, n, 6], sent [T, n] = vwarm[6] after every solve; the vector is carried in registers."""
    return lib().dc_solve6_chain(_p(A), _p(b), lo, hi, _p(x), _p(sent), int(fast), int(mark), int(T), int(n), _stream())


def scalar(v, rcp, rsq, n):
    return lib().dc_scalar(_p(v), _p(rcp), _p(rsq), int(n), _stream())


def trig_chain(dl, sn, cs, K, n):
    """dl [K, n]; sn, cs [n] in/out: K calls of trig_advance per lane."""
    return lib().dc_trig_chain(_p(dl), _p(sn), _p(cs), int(K), int(n), _stream())


def ik_update(des, jpos, jvel, length, ikq_out, tau_out, use_vwarm, use_trig, period, fast, n):
    """des (position + unit quaternion), jpos, jvel [K, n, 7], length [n] int32 -> ikq_out, tau_out [K, n, 7] (rows k < length[e] of lane e are written)."""
    return lib().dc_ik_update(_p(des), _p(jpos), _p(jvel), _p(length), _p(ikq_out), _p(tau_out), int(use_vwarm), int(use_trig), int(period), int(fast), int(n), _stream())


# ---------------------------------------------------------------- leaf routines of the contact engines (f64 tensors; count / hit / ok int32)
def box_box(p1, R1, s1, p2, R2, s2, margin, cap, count, rec, n):
    """p, s [n, 3], R [n, 9] row-major, margin [n] -> count [n] int32, rec [n, 8, 7] (pre-filled by the caller; rows >= count stay)."""
    return lib().dc_box_box(_p(p1), _p(R1), _p(s1), _p(p2), _p(R2), _p(s2), _p(margin), int(cap), _p(count), _p(rec), int(n), _stream())


def cyl_box(pc, axis, par, pb, Rb, sb, hit, out, n):
    """pc, axis, pb, sb [n, 3], par [n, 3] = rad, half, margin, Rb [n, 9] -> hit [n] int32, out [n, 7] (written on a hit only)."""
    return lib().dc_cyl_box(_p(pc), _p(axis), _p(par), _p(pb), _p(Rb), _p(sb), _p(hit), _p(out), int(n), _stream())


def cone_eval(jar, par, out, n):
    """jar [n, 3], par [n, 4] = Dn, Dt, mu, fric -> out [n, 2, 13] = cost, force3, Hc9 of cone_eval and of gt_cone_eval."""
    return lib().dc_cone_eval(_p(jar), _p(par), _p(out), int(n), _stream())


def ldl(order, twin, A, b, L, d, x, ok, n):
    """A, L [n, order (order + 1) / 2], b, d, x [n, order], ok [n] int32."""
    return lib().dc_ldl(int(order), int(twin), _p(A), _p(b), _p(L), _p(d), _p(x), _p(ok), int(n), _stream())


def cube_chain(state, acc, h, K, qhist, n):
    """state [n, 13] in/out, acc [n, 6], h [n]; qhist [K, n, 4] or None."""
    return lib().dc_cube_chain(_p(state), _p(acc), _p(h), int(K), _p(qhist), int(n), _stream())


def tan_yaw(q, out, n):
    return lib().dc_tan_yaw(_p(q), _p(out), int(n), _stream())


def quat2mat(q, R, n):
    return lib().dc_quat2mat(_p(q), _p(R), int(n), _stream())
