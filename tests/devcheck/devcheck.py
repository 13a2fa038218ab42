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
