"""ctypes mirror of the bundle adjustment (include/iba_mi355x.h, iba_bundle*; csrc/iba_bundle.hip): jobs and options, the batch call, the result
object with its accessors, the single linearisation, the host-only plan and the debug hooks. Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last

MAX_FREE_CAMERAS = 64
MAX_ROUNDS = 4


class IbaBundleJob(C.Structure):
    _fields_ = [("Tcw12", C.c_void_p), ("fixed", C.c_void_p), ("xyz", C.c_void_p), ("edge_point", C.c_void_p), ("edge_camera", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("n_cameras", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class IbaBundleOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rounds", C.c_int32), ("iterations", C.c_int32 * MAX_ROUNDS), ("robust_rounds", C.c_int32),
                ("chi2_threshold", C.c_float), ("huber_delta", C.c_float), ("keep_stages", C.c_int32)]


class IbaBundleResult(C.Structure):
    _fields_ = [("n_cameras", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("n_free", C.c_int32), ("n_outliers", C.c_int32), ("rounds_run", C.c_int32),
                ("chi2", C.c_double * MAX_ROUNDS), ("n_bad", C.c_int32 * MAX_ROUNDS), ("lm_iterations", C.c_int32 * MAX_ROUNDS), ("trials", C.c_int32 * MAX_ROUNDS)]


class IbaBundleEvalOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Hpp", "bp", "Hll", "bl", "chi2_edges", "S", "bs", "dp", "dl")] + \
               [("chi2_robust", C.c_double), ("lambda_", C.c_double), ("n_reduced", C.c_int32), ("solved", C.c_int32)]


def _lib():
    L = load_library()
    L.iba_bundle_last_error.restype = C.c_char_p
    L.iba_bundle_last_error.argtypes = []
    L.iba_default_bundle_options.argtypes = [C.c_void_p]
    L.iba_bundle_options_global.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.iba_bundle_optimize.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_debug_bundle_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_bundle_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_int, C.c_void_p]
    L.iba_debug_bundle_eval_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
    L.iba_bundle_free.argtypes = [C.c_void_p]
    L.iba_bundle_free.restype = None
    L.iba_bundle_n_jobs.argtypes = [C.c_void_p]
    L.iba_bundle_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_bundle_cameras.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_bundle_points.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_bundle_edges.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_bundle_stage.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_bundle_plan.argtypes = [C.c_void_p] * 10
    L.iba_bundle_local_window.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 10
    L.iba_debug_bundle_big_steps.argtypes = [C.c_void_p]
    L.iba_debug_bundle_chunks.argtypes = [C.c_void_p]
    L.iba_debug_bundle_kernel_ms.argtypes = [C.c_void_p]
    L.iba_debug_bundle_kernel_ms.restype = C.c_float
    return L


_raise = partial(raise_last, "iba_bundle_last_error")


def options(**fields):
    """iba_default_bundle_options (the local schedule) with fields overridden; iterations takes a sequence of up to 4"""
    L = _lib()
    its = fields.pop("iterations", None)
    o = options_from(IbaBundleOptions, L.iba_default_bundle_options, L.iba_bundle_last_error, **fields)
    if its is not None:
        for k, v in enumerate(its):
            o.iterations[k] = int(v)
    return o


def options_global(n_iterations, robust, **fields):
    """iba_bundle_options_global: one round of n_iterations, the Huber kernel on where robust, with fields overridden"""
    L = _lib()
    o = IbaBundleOptions()
    st = L.iba_bundle_options_global(C.addressof(o), C.c_int32(n_iterations), C.c_int32(1 if robust else 0))
    if st != 0:
        _raise(L, st)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def job(Tcw, fixed, xyz, edge_point, edge_camera, obs, inv_sigma2, K):
    """an IbaBundleJob over copies of the arrays (kept alive by the struct): Tcw [nc, 3, 4] f64, fixed [nc] u8, xyz [np, 3] f32, edge_point and
    edge_camera [ne] i32, obs [ne, 2] f32, inv_sigma2 [ne] f32, K = (fx, fy, cx, cy)"""
    q = IbaBundleJob()
    q._keep = (np.ascontiguousarray(Tcw, np.float64).reshape(-1, 12).copy(), np.ascontiguousarray(fixed, np.uint8).reshape(-1).copy(),
               np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).copy(), np.ascontiguousarray(edge_point, np.int32).reshape(-1).copy(),
               np.ascontiguousarray(edge_camera, np.int32).reshape(-1).copy(), np.ascontiguousarray(obs, np.float32).reshape(-1, 2).copy(),
               np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1).copy())
    T, f, x, ep, ec, ob, w = q._keep
    assert len(T) == len(f) and len(ep) == len(ec) == len(ob) == len(w)
    q.n_cameras, q.n_points, q.n_edges = len(T), len(x), len(ep)
    q.Tcw12, q.fixed = (T.ctypes.data, f.ctypes.data) if len(T) else (None, None)
    q.xyz = x.ctypes.data if len(x) else None
    q.edge_point, q.edge_camera, q.obs, q.inv_sigma2 = (ep.ctypes.data, ec.ctypes.data, ob.ctypes.data, w.ctypes.data) if len(ep) else (None,) * 4
    q.fx, q.fy, q.cx, q.cy = (float(v) for v in K)
    return q


def _job_array(jobs):
    ja = (IbaBundleJob * max(len(jobs), 1))()
    for i, q in enumerate(jobs):
        C.memmove(C.addressof(ja[i]), C.addressof(q), C.sizeof(IbaBundleJob))
    return ja


class Bundle(Result):
    """iba_bundle_batch wrapper: the results of the jobs of one iba_bundle_optimize; close() it"""
    FREE, LAST_ERROR = "iba_bundle_free", "iba_bundle_last_error"

    def __init__(self, lib, p, shapes):
        super().__init__(lib, p)
        self.shapes = shapes

    def __len__(self):
        return int(self.lib.iba_bundle_n_jobs(self.p))

    @property
    def big_steps(self):
        return int(self.lib.iba_debug_bundle_big_steps(self.p))

    @property
    def chunks(self):
        return int(self.lib.iba_debug_bundle_chunks(self.p))

    @property
    def kernel_ms(self):
        """iba_debug_bundle_kernel_ms: 0 unless IBA_BUNDLE_TIMING"""
        return float(self.lib.iba_debug_bundle_kernel_ms(self.p))

    def _shape(self, job):
        return self.shapes[job] if 0 <= job < len(self.shapes) else (0, 0, 0)

    def read(self, job):
        """-> dict of iba_bundle_result: the scalars as Python ints, chi2 [4] f64, n_bad, lm_iterations, trials [4] i32"""
        r = IbaBundleResult()
        self._chk(self.lib.iba_bundle_read(self.p, C.c_int32(job), C.addressof(r)))
        d = {k: int(getattr(r, k)) for k in ("n_cameras", "n_points", "n_edges", "n_free", "n_outliers", "rounds_run")}
        d["chi2"] = np.frombuffer(bytes(r.chi2), np.float64).copy()
        for k in ("n_bad", "lm_iterations", "trials"):
            d[k] = np.array(getattr(r, k)[:], np.int32)
        return d

    def cameras(self, job):
        """-> (Tcw [nc, 3, 4] f64, the same rounded to f32)"""
        nc = self._shape(job)[0]
        T, Tf = np.zeros((nc, 3, 4), np.float64), np.zeros((nc, 3, 4), np.float32)
        self._chk(self.lib.iba_bundle_cameras(self.p, C.c_int32(job), _p(T), _p(Tf)))
        return T, Tf

    def points(self, job):
        """-> (xyz [np, 3] f64, the same rounded to f32)"""
        n = self._shape(job)[1]
        X, Xf = np.zeros((n, 3), np.float64), np.zeros((n, 3), np.float32)
        self._chk(self.lib.iba_bundle_points(self.p, C.c_int32(job), _p(X), _p(Xf)))
        return X, Xf

    def edges(self, job):
        """-> (outlier [ne] u8, chi2 [ne] f32) of the last classification"""
        n = self._shape(job)[2]
        out, chi2 = np.zeros(n, np.uint8), np.zeros(n, np.float32)
        self._chk(self.lib.iba_bundle_edges(self.p, C.c_int32(job), _p(out), _p(chi2)))
        return out, chi2

    def stage(self, job, round):
        """keep_stages -> (Tcw [nc, 3, 4], xyz [np, 3]) f64 at the end of the round"""
        nc, n, _ = self._shape(job)
        T, X = np.zeros((nc, 3, 4), np.float64), np.zeros((n, 3), np.float64)
        self._chk(self.lib.iba_bundle_stage(self.p, C.c_int32(job), C.c_int32(round), _p(T), _p(X)))
        return T, X

    def everything(self, job):
        """every output of a job as a list of (name, array), stages included where kept: what a byte-for-byte comparison walks"""
        r = self.read(job)
        out = [("counts", np.array([r[k] for k in ("n_cameras", "n_points", "n_edges", "n_free", "n_outliers", "rounds_run")], np.int32))]
        out += [(k, r[k]) for k in ("chi2", "n_bad", "lm_iterations", "trials")]
        out += list(zip(("Tcw", "Tcwf"), self.cameras(job))) + list(zip(("xyz", "xyzf"), self.points(job))) + list(zip(("outlier", "edge_chi2"), self.edges(job)))
        for k in range(r["rounds_run"] if self.keep_stages else 0):
            out += list(zip(("stage%d_Tcw" % k, "stage%d_xyz" % k), self.stage(job, k)))
        return out

    keep_stages = False


def _call(jobs, opt, device, host, fields):
    L = _lib()
    o = options(**fields) if opt is None else opt
    ja = _job_array(jobs)
    p = C.c_void_p(None)
    if host:
        st = L.iba_debug_bundle_host(C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o), C.addressof(p))
    else:
        st = L.iba_bundle_optimize(C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o), C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    b = Bundle(L, p, [(int(q.n_cameras), int(q.n_points), int(q.n_edges)) for q in jobs])
    b.keep_stages = bool(o.keep_stages)
    return b


def optimize(jobs, opt=None, device=0, **fields):
    """iba_bundle_optimize: jobs = a list of IbaBundleJob (job()) -> Bundle. opt = an IbaBundleOptions, or fields of one over the local defaults."""
    return _call(jobs, opt, device, False, fields)


def optimize_host(jobs, opt=None, **fields):
    """iba_debug_bundle_host: the same call through the host restatement of the rules, no device"""
    return _call(jobs, opt, 0, True, fields)


EVAL_FIELDS = ("Hpp", "bp", "Hll", "bl", "chi2_edges", "S", "bs", "dp", "dl")


def evaluate(jobs, active=None, robust=True, lam=0.0, device=0, host=False):
    """iba_bundle_eval (host=True: iba_debug_bundle_eval_host): one linearisation per job at its estimates and one step at lambda = lam. active = None
    or a list with None or an [ne] u8 mask per job -> a list of dicts: Hpp [nc, 6, 6], bp [nc, 6], Hll [np, 3, 3], bl [np, 3], chi2_edges [ne], S [n, n]
    (n = n_reduced), bs, dp [nc, 6], dl [np, 3], chi2_robust, lam, n_reduced, solved"""
    L = _lib()
    B = len(jobs)
    ja = _job_array(jobs)
    masks, act = None, None
    if active is not None:
        masks = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in active]
        act = (C.c_void_p * max(B, 1))(*[None if a is None else a.ctypes.data for a in masks])
    outs = (IbaBundleEvalOut * max(B, 1))()
    arrays = []
    for i, q in enumerate(jobs):
        nc, n, ne = int(q.n_cameras), int(q.n_points), int(q.n_edges)
        nf = 6 * min(nc, MAX_FREE_CAMERAS)
        a = dict(Hpp=np.zeros((nc, 6, 6)), bp=np.zeros((nc, 6)), Hll=np.zeros((n, 3, 3)), bl=np.zeros((n, 3)), chi2_edges=np.zeros(ne), S=np.zeros(nf * nf + 1),
                 bs=np.zeros((nc, 6)), dp=np.zeros((nc, 6)), dl=np.zeros((n, 3)))
        for k in EVAL_FIELDS:
            setattr(outs[i], k, a[k].ctypes.data if a[k].size else None)
        arrays.append(a)
    args = [C.addressof(ja), C.c_int32(B), None if act is None else C.addressof(act), C.c_int32(1 if robust else 0), C.c_double(lam)]
    st = L.iba_debug_bundle_eval_host(*args, C.addressof(outs)) if host else L.iba_bundle_eval(*args, C.c_int(device), C.addressof(outs))
    if st != 0:
        _raise(L, st)
    for i, a in enumerate(arrays):
        n = int(outs[i].n_reduced)
        a["S"] = a["S"][:n * n].reshape(n, n).copy()
        a.update(chi2_robust=float(outs[i].chi2_robust), lam=float(outs[i].lambda_), n_reduced=n, solved=int(outs[i].solved))
    return arrays


def plan(q):
    """iba_bundle_plan (host only, rules B6 and B10) of one job -> dict: point_offsets, point_edges, camera_offsets, camera_edges, block_cameras
    [nb, 2], block_offsets [nb + 1], items [ni, 3] (point, edge of a, edge of b), all i32"""
    L = _lib()
    nb, ni = C.c_int32(0), C.c_int32(0)
    st = L.iba_bundle_plan(C.addressof(q), None, None, None, None, C.addressof(nb), C.addressof(ni), None, None, None)
    if st != 0:
        _raise(L, st)
    d = dict(point_offsets=np.zeros(q.n_points + 1, np.int32), point_edges=np.zeros(q.n_edges, np.int32), camera_offsets=np.zeros(q.n_cameras + 1, np.int32),
             camera_edges=np.zeros(q.n_edges, np.int32), block_cameras=np.zeros((nb.value, 2), np.int32), block_offsets=np.zeros(nb.value + 1, np.int32),
             items=np.zeros((ni.value, 3), np.int32))
    st = L.iba_bundle_plan(C.addressof(q), _p(d["point_offsets"]), _p(d["point_edges"]), _p(d["camera_offsets"]), _p(d["camera_edges"]), C.addressof(nb), C.addressof(ni),
                           _p(d["block_cameras"]), _p(d["block_offsets"]), _p(d["items"]))
    if st != 0:
        _raise(L, st)
    return d


def local_window(observations, point_bad, keyframe_bad, current, covisible):
    """iba_bundle_local_window (host only) -> dict: camera_keyframe [nc] i32, fixed [nc] u8, n_local, point_id [np] i32, edge_point, edge_camera,
    edge_keypoint [ne] i32"""
    L = _lib()
    ob = np.ascontiguousarray(observations, np.int32).reshape(-1, 3)
    pb, kb = np.ascontiguousarray(point_bad, np.uint8).reshape(-1), np.ascontiguousarray(keyframe_bad, np.uint8).reshape(-1)
    cv = np.ascontiguousarray(covisible, np.int32).reshape(-1)
    cam, fixed, pid = np.zeros(len(kb) + 1, np.int32), np.zeros(len(kb) + 1, np.uint8), np.zeros(len(pb) + 1, np.int32)
    ep, ec, ek = (np.zeros(len(ob) + 1, np.int32) for _ in range(3))
    n = [C.c_int32(0) for _ in range(4)]
    st = L.iba_bundle_local_window(_p(ob) if len(ob) else None, C.c_int32(len(ob)), _p(pb) if len(pb) else None, C.c_int32(len(pb)), _p(kb) if len(kb) else None,
                                   C.c_int32(len(kb)), C.c_int32(current), _p(cv) if len(cv) else None, C.c_int32(len(cv)), _p(cam), _p(fixed), C.addressof(n[0]),
                                   C.addressof(n[1]), _p(pid), C.addressof(n[2]), _p(ep), _p(ec), _p(ek), C.addressof(n[3]))
    if st != 0:
        _raise(L, st)
    nl, nc, npt, ne = (v.value for v in n)
    return dict(camera_keyframe=cam[:nc], fixed=fixed[:nc], n_local=nl, point_id=pid[:npt], edge_point=ep[:ne], edge_camera=ec[:ne], edge_keypoint=ek[:ne])
