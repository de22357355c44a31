"""ctypes mirror of the robust pose-graph smoother (include/iba_mi355x.h, iba_smooth_*; csrc/iba_smooth.hip): a prior, odometry and robust loop
factors on a graph that grows between updates and stays on the device. Plumbing only."""
import ctypes as C

import numpy as np

from . import IbaError, load_library
from .pgo import STOP  # noqa: F401  (the stops are iba_pgo's)


class IbaSmoothOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_iteration", C.c_int32), ("max_iteration_lm", C.c_int32), ("segment", C.c_int32),
                ("min_relative_increment", C.c_double), ("min_relative_residual_increment", C.c_double), ("min_right_term", C.c_double),
                ("min_residual", C.c_double), ("upper_scale_factor", C.c_double), ("lower_scale_factor", C.c_double)]


class IbaSmoothResult(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_nodes", C.c_int32), ("n_factors", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32),
                ("stop", C.c_int32), ("F_start", C.c_double), ("F", C.c_double), ("lambda_start", C.c_double), ("lambda_", C.c_double), ("max_b", C.c_double)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _lib():
    L = load_library()
    L.iba_smooth_last_error.restype = C.c_char_p
    L.iba_smooth_last_error.argtypes = [C.c_void_p]
    L.iba_smooth_destroy.argtypes = [C.c_void_p]
    L.iba_smooth_destroy.restype = None
    L.iba_default_smooth_options.argtypes = [C.POINTER(IbaSmoothOptions)]
    L.iba_smooth_create.argtypes = [C.POINTER(IbaSmoothOptions), C.c_int, C.POINTER(C.c_void_p)]
    L.iba_smooth_add_node.argtypes = [C.c_void_p, C.c_void_p]
    L.iba_smooth_add_prior.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_smooth_add_between.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    L.iba_smooth_linearize.argtypes = [C.c_void_p] * 6 + [C.POINTER(C.c_double)]
    L.iba_smooth_solve.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    L.iba_smooth_update.argtypes = [C.c_void_p, C.POINTER(IbaSmoothResult)]
    L.iba_smooth_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_debug_smooth_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    return L


def smooth_options(**fields):
    """iba_default_smooth_options with fields overridden"""
    o = IbaSmoothOptions()
    st = _lib().iba_default_smooth_options(C.byref(o))
    if st != 0:
        raise IbaError(st, "iba_default_smooth_options")
    for k, v in fields.items():
        if k not in dict(IbaSmoothOptions._fields_):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _f64(a, n):
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))
    if len(a) != n:
        raise ValueError("expected %d numbers, got %d" % (n, len(a)))
    return a


class Smoother:
    """iba_smooth wrapper. Building the graph needs no device; linearize / solve / update open it."""

    def __init__(self, opt=None, device=0, **fields):
        self.lib = _lib()
        self.opt = smooth_options(**fields) if opt is None else opt
        self.N = self.F = 0
        self.h = C.c_void_p(None)
        st = self.lib.iba_smooth_create(C.byref(self.opt), C.c_int(device), C.byref(self.h))
        if st != 0:
            raise IbaError(st, self.lib.iba_smooth_last_error(None).decode())

    def _chk(self, st):
        if st != 0:
            raise IbaError(st, self.lib.iba_smooth_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.iba_smooth_destroy(self.h)
            self.h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_node(self, pose):
        self._chk(self.lib.iba_smooth_add_node(self.h, _p(_f64(pose, 16))))
        self.N += 1
        return self.N - 1

    def add_prior(self, node, Z, var):
        self._chk(self.lib.iba_smooth_add_prior(self.h, C.c_int32(node), _p(_f64(Z, 16)), _p(_f64(var, 6))))
        self.F += 1

    def add_between(self, i, j, Z, var, robust=False):
        self._chk(self.lib.iba_smooth_add_between(self.h, C.c_int32(i), C.c_int32(j), _p(_f64(Z, 16)), _p(_f64(var, 6)), C.c_int32(int(bool(robust)))))
        self.F += 1

    def linearize(self):
        """-> dict(r [F, 6], w [F], A [F, 6, 6], D [N, 6, 6], b [N, 6], F)"""
        F, N = self.F, self.N
        r, w, A, D, b, Fv = np.zeros((max(F, 1), 6)), np.zeros(max(F, 1)), np.zeros((max(F, 1), 6, 6)), np.zeros((max(N, 1), 6, 6)), np.zeros((max(N, 1), 6)), C.c_double(0.0)
        self._chk(self.lib.iba_smooth_linearize(self.h, _p(r), _p(w), _p(A), _p(D), _p(b), C.byref(Fv)))
        return dict(r=r[:F], w=w[:F], A=A[:F], D=D[:N], b=b[:N], F=Fv.value)

    def solve(self, lam):
        d = np.zeros((max(self.N, 1), 6))
        self._chk(self.lib.iba_smooth_solve(self.h, C.c_double(lam), _p(d)))
        return d[:self.N]

    def update(self):
        r = IbaSmoothResult()
        self._chk(self.lib.iba_smooth_update(self.h, C.byref(r)))
        return r

    def read(self, first=0, count=None):
        """-> (nodes [count, 4, 4], weight [F])"""
        count = self.N - first if count is None else count
        nd, w = np.zeros((max(count, 1), 16)), np.zeros(max(self.F, 1))
        self._chk(self.lib.iba_smooth_read(self.h, C.c_int32(first), C.c_int32(count), _p(nd), _p(w)))
        return nd[:count].reshape(-1, 4, 4), w[:self.F]

    def trace(self):
        """iba_debug_smooth_trace: the trials of the last update: 1 accepted, 0 rejected, 2 stopped on the increment"""
        n = C.c_int32(0)
        self._chk(self.lib.iba_debug_smooth_trace(self.h, None, C.c_int32(0), C.byref(n)))
        t = np.zeros(max(n.value, 1), np.uint8)
        self._chk(self.lib.iba_debug_smooth_trace(self.h, _p(t), C.c_int32(len(t)), C.byref(n)))
        return [int(v) for v in t[:n.value]]
