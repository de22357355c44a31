"""ctypes mirror of the pose-graph optimiser (include/iba_mi355x.h, iba_pgo_*; csrc/iba_pgo.hip): Open3D's GlobalOptimization — LM with line
process, pruning, LM again — on a graph that stays on the device. Plumbing only."""
import ctypes as C

import numpy as np

from . import IbaError, load_library

MAX_SEPARATORS = 1024
STOP = {0: "none", 1: "right_term", 2: "increment", 3: "residual_increment", 4: "residual", 5: "max_iteration"}


class IbaPgoEdge(C.Structure):
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("T", C.c_double * 16), ("info", C.c_double * 36), ("uncertain", C.c_int32)]


class IbaPgoOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reference_node", C.c_int32), ("max_corr_dist", C.c_double), ("edge_prune_threshold", C.c_double),
                ("preference_loop_closure", C.c_double), ("max_iteration", C.c_int32), ("max_iteration_lm", C.c_int32), ("min_relative_increment", C.c_double),
                ("min_relative_residual_increment", C.c_double), ("min_right_term", C.c_double), ("min_residual", C.c_double), ("upper_scale_factor", C.c_double),
                ("lower_scale_factor", C.c_double), ("segment", C.c_int32), ("reserved", C.c_int32)]


class IbaPgoPass(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("stop", C.c_int32), ("reserved", C.c_int32), ("residual", C.c_double), ("lambda_", C.c_double)]


class IbaPgoResult(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pruned", C.c_int32), ("passes", IbaPgoPass * 2)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _lib():
    L = load_library()
    L.iba_pgo_last_error.restype = C.c_char_p
    L.iba_pgo_last_error.argtypes = [C.c_void_p]
    L.iba_pgo_destroy.argtypes = [C.c_void_p]
    L.iba_pgo_destroy.restype = None
    L.iba_pgo_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(IbaPgoOptions), C.c_int, C.POINTER(C.c_void_p)]
    L.iba_pgo_plan.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(IbaPgoOptions), C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32,
                               C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.iba_pgo_linearize.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_double)]
    L.iba_pgo_solve.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    L.iba_pgo_optimize.argtypes = [C.c_void_p, C.POINTER(IbaPgoResult)]
    L.iba_pgo_read.argtypes = [C.c_void_p] * 4
    L.iba_debug_pgo_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    return L


def pgo_options(**fields):
    """iba_default_pgo_options (Open3D's criteria, backend.yml's distances) with fields overridden"""
    o = IbaPgoOptions()
    st = _lib().iba_default_pgo_options(C.byref(o))
    if st != 0:
        raise IbaError(st, "iba_default_pgo_options")
    for k, v in fields.items():
        if k not in dict(IbaPgoOptions._fields_):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def pgo_edges(edges):
    """edges: iterable of (source, target, T 4x4, info 6x6, uncertain) -> (ctypes array of IbaPgoEdge, E)"""
    edges = list(edges)
    arr = (IbaPgoEdge * max(len(edges), 1))()
    for k, (s, t, T, info, unc) in enumerate(edges):
        arr[k].source, arr[k].target, arr[k].uncertain = int(s), int(t), int(bool(unc))
        arr[k].T[:] = np.asarray(T, np.float64).reshape(16).tolist()
        arr[k].info[:] = np.asarray(info, np.float64).reshape(36).tolist()
    return arr, len(edges)


def pgo_plan(N, edges, opt=None, **fields):
    """iba_pgo_plan (host only): -> dict(separators [S], runs [R, 2] (first, last), K)"""
    L = _lib()
    o = pgo_options(**fields) if opt is None else opt
    arr, E = edges if isinstance(edges, tuple) else pgo_edges(edges)
    sep = np.zeros(max(int(N), 1), np.int32)
    runs = np.zeros((max(int(N), 1), 2), np.int32)
    ns, nr, K = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    st = L.iba_pgo_plan(C.c_int32(N), arr, C.c_int32(E), C.byref(o), _p(sep), C.c_int32(len(sep)), C.byref(ns), _p(runs), C.c_int32(len(runs)), C.byref(nr), C.byref(K))
    if st != 0:
        raise IbaError(st, L.iba_pgo_last_error(None).decode())
    return dict(separators=sep[:ns.value].copy(), runs=runs[:nr.value].copy(), K=K.value)


class PoseGraph:
    """iba_pgo wrapper. nodes [N, 4, 4]; edges as for pgo_edges (or its result); opt an IbaPgoOptions or fields over the defaults."""

    def __init__(self, nodes, edges, opt=None, device=0, **fields):
        self.lib = _lib()
        self.opt = pgo_options(**fields) if opt is None else opt
        nd = np.ascontiguousarray(np.asarray(nodes, np.float64).reshape(-1, 16))
        self.N = len(nd)
        arr, self.E = edges if isinstance(edges, tuple) else pgo_edges(edges)
        self.h = C.c_void_p(None)
        st = self.lib.iba_pgo_create(_p(nd), C.c_int32(self.N), arr, C.c_int32(self.E), C.byref(self.opt), C.c_int(device), C.byref(self.h))
        if st != 0:
            raise IbaError(st, self.lib.iba_pgo_last_error(None).decode())

    def _chk(self, st):
        if st != 0:
            raise IbaError(st, self.lib.iba_pgo_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.iba_pgo_destroy(self.h)
            self.h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def linearize(self):
        """-> dict(zeta [E, 6], weight [E], A [E, 6, 6], b [N, 6], residual)"""
        E, N = self.E, self.N
        z, w, A, b, r = np.zeros((max(E, 1), 6)), np.zeros(max(E, 1)), np.zeros((max(E, 1), 6, 6)), np.zeros((N, 6)), C.c_double(0.0)
        self._chk(self.lib.iba_pgo_linearize(self.h, _p(z), _p(w), _p(A), _p(b), C.byref(r)))
        return dict(zeta=z[:E], weight=w[:E], A=A[:E], b=b, residual=r.value)

    def solve(self, lam):
        d = np.zeros((self.N, 6))
        self._chk(self.lib.iba_pgo_solve(self.h, C.c_double(lam), _p(d)))
        return d

    def optimize(self):
        r = IbaPgoResult()
        self._chk(self.lib.iba_pgo_optimize(self.h, C.byref(r)))
        return r

    def read(self):
        """-> (nodes [N, 4, 4], weight [E], pruned [E] bool)"""
        nd, w, pr = np.zeros((self.N, 16)), np.zeros(max(self.E, 1)), np.zeros(max(self.E, 1), np.uint8)
        self._chk(self.lib.iba_pgo_read(self.h, _p(nd), _p(w), _p(pr)))
        return nd.reshape(-1, 4, 4), w[:self.E], pr[:self.E].astype(bool)

    def trace(self):
        """iba_debug_pgo_trace: the trials of the last optimize as (pass, code) with code 1 accepted, 0 rejected, 2 stopped on the increment"""
        n = C.c_int32(0)
        self._chk(self.lib.iba_debug_pgo_trace(self.h, None, C.c_int32(0), C.byref(n)))
        t = np.zeros(max(n.value, 1), np.uint8)
        self._chk(self.lib.iba_debug_pgo_trace(self.h, _p(t), C.c_int32(len(t)), C.byref(n)))
        return [(int(v) >> 7, int(v) & 0x7F) for v in t[:n.value]]
