"""ctypes mirror of the two-view initialisation (include/iba_mi355x.h, iba_twoview*; csrc/iba_twoview.hip): pairs and options, the batch call, the
result object with its stage accessors, the two host-only builders and the debug hooks. Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last

OK, TOO_FEW_MATCHES, NO_MODEL, H_DEGENERATE, NO_CLEAR_WINNER, TOO_FEW_POINTS, LOW_PARALLAX = range(7)
STATUS_NAMES = ("OK", "TOO_FEW_MATCHES", "NO_MODEL", "H_DEGENERATE", "NO_CLEAR_WINNER", "TOO_FEW_POINTS", "LOW_PARALLAX")
MAX_ITERATIONS = 4096


class IbaTwoviewPair(C.Structure):
    _fields_ = [("xy1", C.c_void_p), ("xy2", C.c_void_p), ("matches12", C.c_void_p), ("sets", C.c_void_p), ("n1", C.c_int32), ("n2", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class IbaTwoviewOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("sigma", C.c_float), ("iterations", C.c_int32), ("min_parallax_deg", C.c_float), ("min_triangulated", C.c_int32),
                ("rh_threshold", C.c_float), ("keep_stages", C.c_int32)]


class IbaTwoviewResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("model", C.c_int32), ("n_hyp", C.c_int32), ("chosen", C.c_int32), ("best_it_H", C.c_int32),
                ("best_it_F", C.c_int32), ("n_inliers_H", C.c_int32), ("n_inliers_F", C.c_int32), ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("n_good", C.c_int32 * 8), ("cos_parallax", C.c_float * 8), ("parallax_deg", C.c_float * 8),
                ("R21", C.c_float * 9), ("t21", C.c_float * 3)]


SCALARS = ("status", "n_matches", "model", "n_hyp", "chosen", "best_it_H", "best_it_F", "n_inliers_H", "n_inliers_F", "SH", "SF", "RH")
ARRAYS = ("H21", "F21", "n_good", "cos_parallax", "parallax_deg", "R21", "t21")


def _lib():
    L = load_library()
    L.iba_twoview_last_error.restype = C.c_char_p
    L.iba_twoview_last_error.argtypes = []
    L.iba_default_twoview_options.argtypes = [C.c_void_p]
    L.iba_twoview_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_debug_twoview_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_twoview_free.argtypes = [C.c_void_p]
    L.iba_twoview_free.restype = None
    L.iba_twoview_n_pairs.argtypes = [C.c_void_p]
    L.iba_twoview_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_twoview_matches.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_twoview_points.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_twoview_iterations.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    L.iba_twoview_hypothesis.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    L.iba_twoview_normalize.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_twoview_sets.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]
    L.iba_debug_twoview_null_vector.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_debug_twoview_sweep_cap_hits.argtypes = [C.c_void_p]
    L.iba_debug_twoview_chunks.argtypes = [C.c_void_p]
    L.iba_debug_twoview_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_twoview_last_error")


def options(**fields):
    """iba_default_twoview_options with fields overridden"""
    L = _lib()
    return options_from(IbaTwoviewOptions, L.iba_default_twoview_options, L.iba_twoview_last_error, **fields)


def pair(xy1, xy2, matches12, K, sets=None):
    """an IbaTwoviewPair over copies of the arrays (kept alive by the struct): xy1 [n1, 2] f32, xy2 [n2, 2] f32, matches12 [n1] i32, K = (fx, fy, cx,
    cy), sets [iterations, 8] i32 or None (legal only where fewer than 8 entries of matches12 are >= 0)"""
    p = IbaTwoviewPair()
    p._keep = (np.ascontiguousarray(xy1, np.float32).reshape(-1, 2), np.ascontiguousarray(xy2, np.float32).reshape(-1, 2), np.ascontiguousarray(matches12, np.int32).reshape(-1),
               None if sets is None else np.ascontiguousarray(sets, np.int32).reshape(-1, 8))
    a, b, m, s = p._keep
    assert len(m) == len(a)
    p.n1, p.n2 = len(a), len(b)
    p.xy1, p.matches12 = (a.ctypes.data, m.ctypes.data) if len(a) else (None, None)
    p.xy2 = b.ctypes.data if len(b) else None
    p.sets = s.ctypes.data if s is not None and len(s) else None
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in K)
    return p


def normalize(xy):
    """iba_twoview_normalize (host only, rule T1) -> (out_xy [n, 2] f32, T [3, 3] f32)"""
    L = _lib()
    a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out, T = np.zeros_like(a), np.zeros((3, 3), np.float32)
    st = L.iba_twoview_normalize(_p(a), C.c_int32(len(a)), _p(out), _p(T))
    if st != 0:
        _raise(L, st)
    return out, T


def sets(N, iterations, seed):
    """iba_twoview_sets (host only) -> [iterations, 8] i32"""
    L = _lib()
    out = np.zeros((max(iterations, 0), 8), np.int32)
    st = L.iba_twoview_sets(C.c_int32(N), C.c_int32(iterations), C.c_uint64(seed), _p(out))
    if st != 0:
        _raise(L, st)
    return out


def null_vector(A):
    """iba_debug_twoview_null_vector (host only, rule T2) on a float32 matrix of 16 x 9, 8 x 9, 4 x 4 or 3 x 3 -> (v [n] f32, the float64 column it was
    rounded from, sweeps)"""
    L = _lib()
    a = np.ascontiguousarray(A, np.float32)
    v, v64, sw = np.zeros(a.shape[1], np.float32), np.zeros(a.shape[1], np.float64), C.c_int32(0)
    st = L.iba_debug_twoview_null_vector(_p(a), C.c_int32(a.shape[0]), C.c_int32(a.shape[1]), _p(v), _p(v64), C.addressof(sw))
    if st != 0:
        _raise(L, st)
    return v, v64, sw.value


class Twoview(Result):
    """iba_twoview_batch wrapper: the results of the pairs of one iba_twoview_init; close() it"""
    FREE, LAST_ERROR = "iba_twoview_free", "iba_twoview_last_error"

    def __init__(self, lib, p, n1, iterations):
        super().__init__(lib, p)
        self.n1, self.iterations = n1, iterations

    def __len__(self):
        return int(self.lib.iba_twoview_n_pairs(self.p))

    @property
    def chunks(self):
        """iba_debug_twoview_chunks: the chunks the call ran as; 0 on the host"""
        return int(self.lib.iba_debug_twoview_chunks(self.p))

    @property
    def sweep_cap_hits(self):
        return int(self.lib.iba_debug_twoview_sweep_cap_hits(self.p))

    @property
    def stage_ms(self):
        """iba_debug_twoview_stage_ms: (hypotheses, scores, selection, motion, CheckRT, k-th cosine, acceptance) in ms; zeros unless IBA_TWOVIEW_TIMING"""
        ms = np.zeros(7, np.float32)
        self._chk(self.lib.iba_debug_twoview_stage_ms(self.p, _p(ms)))
        return ms

    def read(self, pair):
        """-> dict of iba_twoview_result: the scalars as Python numbers, the arrays as numpy arrays (H21, F21, R21 as [3, 3])"""
        r = IbaTwoviewResult()
        self._chk(self.lib.iba_twoview_read(self.p, C.c_int32(pair), C.addressof(r)))
        d = {k: getattr(r, k) for k in SCALARS}
        for k in ("SH", "SF", "RH"):
            d[k] = np.float32(d[k])
        for k in ARRAYS:
            a = np.array(getattr(r, k)[:], np.int32 if k == "n_good" else np.float32)
            d[k] = a.reshape(3, 3) if len(a) == 9 else a
        return d

    def matches(self, pair):
        """-> (list [N, 2] i32, inlier [N] u8 of the chosen model)"""
        n = self.read(pair)["n_matches"]
        lst, inl = np.zeros((n, 2), np.int32), np.zeros(n, np.uint8)
        self._chk(self.lib.iba_twoview_matches(self.p, C.c_int32(pair), _p(lst), _p(inl)))
        return lst, inl

    def points(self, pair):
        """-> (points [n1, 3] f32, triangulated [n1] u8) of the chosen motion hypothesis"""
        n1 = self.n1[pair] if 0 <= pair < len(self.n1) else 0
        pts, tri = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
        self._chk(self.lib.iba_twoview_points(self.p, C.c_int32(pair), _p(pts), _p(tri)))
        return pts, tri

    def iterations_of(self, pair):
        """keep_stages -> dict: Hi, H12i, Fi [iterations, 3, 3] f32, score_H, score_F [iterations] f32"""
        n = self.iterations
        d = {"Hi": np.zeros((n, 3, 3), np.float32), "H12i": np.zeros((n, 3, 3), np.float32), "Fi": np.zeros((n, 3, 3), np.float32), "score_H": np.zeros(n, np.float32),
             "score_F": np.zeros(n, np.float32)}
        self._chk(self.lib.iba_twoview_iterations(self.p, C.c_int32(pair), *[_p(d[k]) for k in ("Hi", "H12i", "Fi", "score_H", "score_F")]))
        return d

    def hypothesis(self, pair, hyp):
        """keep_stages -> dict: R [3, 3], t [3], n_good, points [N, 3] f32, verdict [N] u8"""
        n = self.read(pair)["n_matches"] if 0 <= pair < len(self.n1) else 0
        R, t, ng, pts, ver = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), C.c_int32(0), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
        self._chk(self.lib.iba_twoview_hypothesis(self.p, C.c_int32(pair), C.c_int32(hyp), _p(R), _p(t), C.addressof(ng), _p(pts), _p(ver)))
        return {"R": R, "t": t, "n_good": ng.value, "points": pts, "verdict": ver}


def _call(pairs, opt, device, host, fields):
    L = _lib()
    o = options(**fields) if opt is None else opt
    pa = (IbaTwoviewPair * max(len(pairs), 1))()
    for i, q in enumerate(pairs):
        C.memmove(C.addressof(pa[i]), C.addressof(q), C.sizeof(IbaTwoviewPair))
    p = C.c_void_p(None)
    if host:
        st = L.iba_debug_twoview_host(C.addressof(pa), C.c_int32(len(pairs)), C.addressof(o), C.addressof(p))
    else:
        st = L.iba_twoview_init(C.addressof(pa), C.c_int32(len(pairs)), C.addressof(o), C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return Twoview(L, p, [int(q.n1) for q in pairs], int(o.iterations))


def init(pairs, opt=None, device=0, **fields):
    """iba_twoview_init: pairs = a list of IbaTwoviewPair (pair()) -> Twoview. opt = an IbaTwoviewOptions, or fields of one over the defaults."""
    return _call(pairs, opt, device, False, fields)


def init_host(pairs, opt=None, **fields):
    """iba_debug_twoview_host: the same call through the host restatement of the rules, no device"""
    return _call(pairs, opt, 0, True, fields)
