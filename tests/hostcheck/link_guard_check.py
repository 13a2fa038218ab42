"""ctypes loader for the TEST-ONLY host build of the link-near guard (tests/hostcheck/link_guard_check.cpp), built like hostcheck.py."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build(force=False):
    so = os.path.join(_HERE, "libd3il_link_guard_check.so")
    srcs = [os.path.join(_HERE, "link_guard_check.cpp")] + [os.path.join(_HERE, "..", "..", "d3il_amd", "csrc", f) for f in ("link_guard.h", "panda_step.h", "panda_consts.h", "rigid_common.h", "gen_step.h", "gen_tree.h")]
    srcs.append(os.path.join(_HERE, "..", "..", "include", "d3il_model_blob.h"))
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]])
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.lgc_create.restype = C.c_void_p
        _LIB.lgc_slack.restype = C.c_double
        _LIB.lgc_seg_box.restype = C.c_double
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class LinkGuardHost:
    """The guard of one environment on the CPU: set(capsules [n, 9], margin) as d3il_set_link_guard, eval(q9, cubes [nb, 7]) -> (raised, placed capsules, bound)."""

    def __init__(self, blob):
        self.L = lib()
        err = C.c_char_p()
        self.h = C.c_void_p(self.L.lgc_create(C.byref(blob), C.byref(err)))
        if not self.h:
            raise RuntimeError("lgc_create: %s" % (err.value.decode() if err.value else "?"))
        self.slack = float(self.L.lgc_slack())
        self.n = 0
        nb, ns = C.c_int(0), C.c_int(0)
        st, bh = np.zeros((32, 15)), np.zeros(3)
        self.L.lgc_info(self.h, C.byref(nb), C.byref(ns), _p(st), _p(bh))
        self.nb, self.ns, self.box_half = nb.value, ns.value, bh
        self.st_c, self.st_h, self.st_R = st[:ns.value, 0:3].copy(), st[:ns.value, 3:6].copy(), st[:ns.value, 6:15].reshape(-1, 3, 3).copy()

    def set(self, capsules, margin):
        caps = np.ascontiguousarray(capsules, dtype=np.float64).reshape(-1, 9)
        err = C.c_char_p()
        rc = self.L.lgc_set(self.h, _p(caps) if len(caps) else None, len(caps), C.c_double(margin), C.byref(err))
        if rc:
            raise ValueError(err.value.decode())
        self.n = len(caps)

    def eval(self, q, cubes):
        q, cubes = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(cubes, dtype=np.float64).reshape(self.nb, 7)
        wc, dm = np.zeros((max(self.n, 1), 7)), C.c_double(0)
        raised = self.L.lgc_eval(self.h, _p(q), _p(cubes), _p(wc), C.byref(dm))
        return bool(raised), wc[:self.n], dm.value

    def seg_box(self, a, b, c, R, h):
        """The kernel's lower bound of distance(segment a b, box c / R / h) with the cull switched off."""
        a, b, c, R, h = (np.ascontiguousarray(x, dtype=np.float64) for x in (a, b, c, R, h))
        return float(self.L.lgc_seg_box(_p(a), _p(b), _p(c), _p(R), _p(h)))

    def __del__(self):
        try:
            self.L.lgc_destroy(self.h)
        except Exception:
            pass
