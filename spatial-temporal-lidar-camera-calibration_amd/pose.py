"""ctypes mirror of the motion-only pose optimisation (include/iba_mi355x.h, iba_pose*; csrc/iba_pose.hip): jobs and options, the batch call, the
result object with its accessors, the single linearisation, the host-only edge builder and the debug hooks. Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last

ONCHIP_EDGES = 1024
MAX_ROUNDS = 8


class IbaPoseJob(C.Structure):
    _fields_ = [("Tcw12", C.c_void_p), ("xyz", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p), ("n", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class IbaPoseOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rounds", C.c_int32), ("iterations", C.c_int32), ("chi2_threshold", C.c_float), ("huber_delta", C.c_float),
                ("robust_rounds", C.c_int32), ("keep_stages", C.c_int32)]


class IbaPoseResult(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_inliers", C.c_int32), ("rounds_run", C.c_int32), ("reserved", C.c_int32), ("Tcw12", C.c_double * 12), ("Tcw12f", C.c_float * 12),
                ("chi2", C.c_double * MAX_ROUNDS), ("n_bad", C.c_int32 * MAX_ROUNDS), ("lm_iterations", C.c_int32 * MAX_ROUNDS), ("trials", C.c_int32 * MAX_ROUNDS)]


def _lib():
    L = load_library()
    L.iba_pose_last_error.restype = C.c_char_p
    L.iba_pose_last_error.argtypes = []
    L.iba_default_pose_options.argtypes = [C.c_void_p]
    L.iba_pose_optimize.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_debug_pose_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_pose_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int] + [C.c_void_p] * 4
    L.iba_debug_pose_eval_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    L.iba_pose_free.argtypes = [C.c_void_p]
    L.iba_pose_free.restype = None
    L.iba_pose_n_jobs.argtypes = [C.c_void_p]
    L.iba_pose_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_pose_edges.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_pose_stage.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.iba_pose_edges_from_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    L.iba_debug_pose_series.argtypes = [C.c_double, C.c_void_p]
    L.iba_debug_pose_exp.argtypes = [C.c_void_p] * 4
    L.iba_debug_pose_big_steps.argtypes = [C.c_void_p]
    L.iba_debug_pose_chunks.argtypes = [C.c_void_p]
    L.iba_debug_pose_kernel_ms.argtypes = [C.c_void_p]
    L.iba_debug_pose_kernel_ms.restype = C.c_float
    return L


_raise = partial(raise_last, "iba_pose_last_error")


def options(**fields):
    """iba_default_pose_options with fields overridden"""
    L = _lib()
    return options_from(IbaPoseOptions, L.iba_default_pose_options, L.iba_pose_last_error, **fields)


def job(Tcw, xyz, obs, inv_sigma2, K):
    """an IbaPoseJob over copies of the arrays (kept alive by the struct): Tcw [3, 4] f64, xyz [n, 3] f32, obs [n, 2] f32, inv_sigma2 [n] f32,
    K = (fx, fy, cx, cy)"""
    q = IbaPoseJob()
    q._keep = (np.ascontiguousarray(Tcw, np.float64).reshape(12).copy(), np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).copy(),
               np.ascontiguousarray(obs, np.float32).reshape(-1, 2).copy(), np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1).copy())
    T, a, b, w = q._keep
    assert len(a) == len(b) == len(w)
    q.n = len(a)
    q.Tcw12 = T.ctypes.data
    q.xyz, q.obs, q.inv_sigma2 = (a.ctypes.data, b.ctypes.data, w.ctypes.data) if len(a) else (None, None, None)
    q.fx, q.fy, q.cx, q.cy = (float(v) for v in K)
    return q


def _job_array(jobs):
    ja = (IbaPoseJob * max(len(jobs), 1))()
    for i, q in enumerate(jobs):
        C.memmove(C.addressof(ja[i]), C.addressof(q), C.sizeof(IbaPoseJob))
    return ja


class Pose(Result):
    """iba_pose_batch wrapper: the results of the jobs of one iba_pose_optimize; close() it"""
    FREE, LAST_ERROR = "iba_pose_free", "iba_pose_last_error"

    def __init__(self, lib, p, n):
        super().__init__(lib, p)
        self.n = n

    def __len__(self):
        return int(self.lib.iba_pose_n_jobs(self.p))

    @property
    def big_steps(self):
        return int(self.lib.iba_debug_pose_big_steps(self.p))

    @property
    def chunks(self):
        return int(self.lib.iba_debug_pose_chunks(self.p))

    @property
    def kernel_ms(self):
        """iba_debug_pose_kernel_ms: 0 unless IBA_POSE_TIMING"""
        return float(self.lib.iba_debug_pose_kernel_ms(self.p))

    def read(self, job):
        """-> dict of iba_pose_result: the scalars as Python ints, Tcw12 [3, 4] f64, Tcw12f [3, 4] f32, chi2 [8] f64, n_bad, lm_iterations, trials [8] i32"""
        r = IbaPoseResult()
        self._chk(self.lib.iba_pose_read(self.p, C.c_int32(job), C.addressof(r)))
        d = {k: int(getattr(r, k)) for k in ("n", "n_inliers", "rounds_run")}
        d["Tcw12"] = np.array(r.Tcw12[:], np.float64).reshape(3, 4)
        d["Tcw12f"] = np.array(r.Tcw12f[:], np.float32).reshape(3, 4)
        d["chi2"] = np.frombuffer(bytes(r.chi2), np.float64).copy()
        for k in ("n_bad", "lm_iterations", "trials"):
            d[k] = np.array(getattr(r, k)[:], np.int32)
        return d

    def edges(self, job):
        """-> (outlier [n] u8, chi2 [n] f32) of the last classification"""
        n = self.n[job] if 0 <= job < len(self.n) else 0
        out, chi2 = np.zeros(n, np.uint8), np.zeros(n, np.float32)
        self._chk(self.lib.iba_pose_edges(self.p, C.c_int32(job), _p(out), _p(chi2)))
        return out, chi2

    def stage(self, job, round):
        """keep_stages -> the pose [3, 4] f64 at the end of the round"""
        T = np.zeros((3, 4), np.float64)
        self._chk(self.lib.iba_pose_stage(self.p, C.c_int32(job), C.c_int32(round), _p(T)))
        return T


def _call(jobs, opt, device, host, fields):
    L = _lib()
    o = options(**fields) if opt is None else opt
    ja = _job_array(jobs)
    p = C.c_void_p(None)
    if host:
        st = L.iba_debug_pose_host(C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o), C.addressof(p))
    else:
        st = L.iba_pose_optimize(C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o), C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return Pose(L, p, [int(q.n) for q in jobs])


def optimize(jobs, opt=None, device=0, **fields):
    """iba_pose_optimize: jobs = a list of IbaPoseJob (job()) -> Pose. opt = an IbaPoseOptions, or fields of one over the defaults."""
    return _call(jobs, opt, device, False, fields)


def optimize_host(jobs, opt=None, **fields):
    """iba_debug_pose_host: the same call through the host restatement of the rules, no device"""
    return _call(jobs, opt, 0, True, fields)


def evaluate(jobs, active=None, robust=True, device=0, chi2_edges=True, host=False):
    """iba_pose_eval (host=True: iba_debug_pose_eval_host): one linearisation per job at its pose. active = None or a list with None or an [n] u8
    mask per job -> (H [B, 6, 6], b [B, 6], chi2_robust [B], a list of per-edge chi2 [n] f64, or None)"""
    L = _lib()
    B = len(jobs)
    ja = _job_array(jobs)
    H, b, c = np.zeros((max(B, 1), 6, 6)), np.zeros((max(B, 1), 6)), np.zeros(max(B, 1))
    masks, act = None, None
    if active is not None:
        masks = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in active]
        act = (C.c_void_p * max(B, 1))(*[None if a is None else a.ctypes.data for a in masks])
    per, ptrs = None, None
    if chi2_edges:
        per = [np.zeros(int(q.n), np.float64) for q in jobs]
        ptrs = (C.c_void_p * max(B, 1))(*[a.ctypes.data if len(a) else None for a in per])
    args = [C.addressof(ja), C.c_int32(B), None if act is None else C.addressof(act), C.c_int32(1 if robust else 0)]
    tail = [_p(H), _p(b), _p(c), None if ptrs is None else C.addressof(ptrs)]
    st = L.iba_debug_pose_eval_host(*args, *tail) if host else L.iba_pose_eval(*args, C.c_int(device), *tail)
    if st != 0:
        _raise(L, st)
    return H[:B], b[:B], c[:B], per


def edges_from_matches(match, query_index, last_world_xyz, cur_xy, cur_octave, inv_level_sigma2):
    """iba_pose_edges_from_matches (host only, rule P9) -> (xyz [n, 3] f32, obs [n, 2] f32, inv_sigma2 [n] f32, keypoint_index [n] i32)"""
    L = _lib()
    m = np.ascontiguousarray(match, np.int32).reshape(-1)
    qi = None if query_index is None else np.ascontiguousarray(query_index, np.int32).reshape(-1)
    wx = np.ascontiguousarray(last_world_xyz, np.float32).reshape(-1, 3)
    xy = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
    oc = np.ascontiguousarray(cur_octave, np.int32).reshape(-1)
    lv = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    assert len(oc) == len(xy) and (qi is None or len(qi) == len(m))
    nc = len(xy)
    xyz, obs, w, idx, n = np.zeros((nc, 3), np.float32), np.zeros((nc, 2), np.float32), np.zeros(nc, np.float32), np.zeros(nc, np.int32), C.c_int32(0)
    st = L.iba_pose_edges_from_matches(_p(m) if len(m) else None, _p(qi) if qi is not None and len(qi) else None, C.c_int32(len(m)), _p(wx) if len(wx) else None, C.c_int32(len(wx)),
                                       _p(xy) if nc else None, _p(oc) if nc else None, C.c_int32(nc), _p(lv) if len(lv) else None, C.c_int32(len(lv)),
                                       _p(xyz) if nc else None, _p(obs) if nc else None, _p(w) if nc else None, _p(idx) if nc else None, C.addressof(n))
    if st != 0:
        _raise(L, st)
    return xyz[:n.value], obs[:n.value], w[:n.value], idx[:n.value]


def series(s):
    """iba_debug_pose_series (host only, rule P6) at s = theta^2 <= pi^2 -> [3] f64"""
    L = _lib()
    out = np.zeros(3, np.float64)
    st = L.iba_debug_pose_series(C.c_double(s), _p(out))
    if st != 0:
        _raise(L, st)
    return out


def exp_update(dx, T):
    """iba_debug_pose_exp (host only, rule P6) -> (Exp(dx) T [3, 4] f64, big)"""
    L = _lib()
    d, t = np.ascontiguousarray(dx, np.float64).reshape(6), np.ascontiguousarray(T, np.float64).reshape(12)
    Tn, big = np.zeros((3, 4), np.float64), C.c_int32(0)
    st = L.iba_debug_pose_exp(_p(d), _p(t), _p(Tn), C.addressof(big))
    if st != 0:
        _raise(L, st)
    return Tn, big.value
