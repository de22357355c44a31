"""MI355X-native IBA cross-modality evaluation path — Python plumbing around the C-ABI library.

The product is csrc/ (hand-written HIP for gfx950 behind include/iba_mi355x.h). This module only
builds/loads libiba_mi355x.so and wraps the entry points with numpy arrays for tests and bench.py.
It never computes anything itself and never touches oracle/: if the HIP library (or a GPU) is
missing, calls fail loudly.

The directory name carries a hyphen; import it with
    importlib.import_module("spatial-temporal-lidar-camera-calibration_amd")
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .abi import (ICP_NMOM, SCAN_NMOM, IbaFloamOptions, IbaScOptions, IbaScQuery, IbaScResult, IbaSubmapDesc, IbaScanEdge, IbaScanOptions, IbaScanResult, IbaIcpOptions, IbaIcpResult, IBA_MAX_BATCH, IbaCreateOptions, IbaLmOptions, IbaLmResult, IbaMadsOptions, IbaMadsResult, IbaBbo, IbaCostOut, IbaNormalOut, IbaParams, IbaProblemDesc, Problem, copy_params,
                  reference_yaml_params)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IBA_LIB", os.path.join(_HERE, "libiba_mi355x.so"))  # IBA_LIB: diagnostic builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "iba_mi355x.h")
# every header of the boundary: the product surface and the diagnostics (tests check that the library exports all they declare)
HEADER_PATHS = [HEADER_PATH, os.path.join(os.path.dirname(_HERE), "include", "iba_mi355x_debug.h")]

STATUS = {0: "IBA_OK", 1: "IBA_ERR_INVALID_ARG", 2: "IBA_ERR_NO_DEVICE", 3: "IBA_ERR_HIP", 4: "IBA_ERR_UNSUPPORTED", 5: "IBA_ERR_STATE", 6: "IBA_ERR_IO"}


class IbaError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS.get(status, status)}: {msg}")
        self.status = status


def build_extension(force=False):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU). Returns the .so path."""
    src_dir = os.path.join(_HERE, "csrc")
    # make tracks the dependencies itself (every .hip / .cpp / .hpp of csrc and the public header)
    if force:
        subprocess.check_call(["make", "-C", src_dir, "-s", "-B"])
    else:
        subprocess.check_call(["make", "-C", src_dir, "-s"])
    return LIB_PATH


_lib = None
ABI_VERSION = 4   # IBA_ABI_VERSION of include/iba_mi355x.h these ctypes structs mirror


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IbaError(2, f"{LIB_PATH} is not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.iba_abi_version.restype = C.c_int32
        if L.iba_abi_version() != ABI_VERSION:   # iba_params has no struct_size: a stale library would read past (or short of) the struct
            raise IbaError(1, f"{LIB_PATH} speaks ABI {L.iba_abi_version()}, these bindings ABI {ABI_VERSION}: rebuild the library")
        L.iba_last_error.restype = C.c_char_p
        L.iba_last_error.argtypes = [C.c_void_p]
        L.iba_create.argtypes = [C.POINTER(IbaProblemDesc), C.POINTER(IbaParams), C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.iba_create_ex.argtypes = [C.POINTER(IbaProblemDesc), C.POINTER(IbaParams), C.c_int, C.c_int32, C.c_int32, C.POINTER(IbaCreateOptions), C.POINTER(C.c_void_p)]
        L.iba_destroy.argtypes = [C.c_void_p]
        L.iba_num_points.restype = C.c_int64
        L.iba_num_points.argtypes = [C.c_void_p]
        L.iba_num_keypoints.restype = C.c_int64
        L.iba_num_keypoints.argtypes = [C.c_void_p]
        L.iba_eval_cost_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.iba_eval_normal_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.iba_eval_full_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.iba_eval_factors_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.iba_comm_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def default_params():
    p = IbaParams()
    load_library().iba_default_params(C.byref(p))
    return p


def create_options(**fields):
    """iba_default_create_options with fields overridden (engine options: none changes a result bit)"""
    o = IbaCreateOptions()
    load_library().iba_default_create_options(C.byref(o))
    for k, v in fields.items():
        if k not in dict(IbaCreateOptions._fields_):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def partial_stride():
    return int(load_library().iba_partial_stride())


def finalize_cost(params, partials):
    partials = np.ascontiguousarray(partials, np.float64).reshape(-1, partial_stride())
    B = len(partials)
    out = (IbaCostOut * B)()
    st = load_library().iba_finalize_cost(C.byref(params), _p(partials), C.c_int32(B), out)
    if st != 0:
        raise IbaError(st, "iba_finalize_cost")
    return list(out)


def finalize_normal(params, partials):
    partials = np.ascontiguousarray(partials, np.float64).reshape(-1, partial_stride())
    B = len(partials)
    out = (IbaNormalOut * B)()
    st = load_library().iba_finalize_normal(C.byref(params), _p(partials), C.c_int32(B), out)
    if st != 0:
        raise IbaError(st, "iba_finalize_normal")
    return list(out)


class IbaHandle:
    """iba_handle wrapper. One evaluation at a time per handle (as BALoss::eval_x)."""

    def __init__(self, problem, params=None, device=0, frame_begin=0, frame_end=None, options=None):
        """options: an IbaCreateOptions (create_options(...)) or a dict of its fields; None = the defaults (iba_create)"""
        self.lib = load_library()
        self.problem = problem
        self.params = copy_params(params) if params is not None else default_params()
        self._desc = problem.desc()
        self.h = C.c_void_p(None)
        fe = problem.n_frames if frame_end is None else frame_end
        self.frame_begin, self.frame_end = frame_begin, fe
        if options is None:
            st = self.lib.iba_create(C.byref(self._desc), C.byref(self.params), C.c_int(device), C.c_int32(frame_begin), C.c_int32(fe), C.byref(self.h))
        else:
            self.options = create_options(**options) if isinstance(options, dict) else options
            st = self.lib.iba_create_ex(C.byref(self._desc), C.byref(self.params), C.c_int(device), C.c_int32(frame_begin), C.c_int32(fe), C.byref(self.options), C.byref(self.h))
        if st != 0:
            raise IbaError(st, self.lib.iba_last_error(None).decode())

    def _chk(self, st):
        if st != 0:
            raise IbaError(st, self.lib.iba_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.iba_destroy(self.h)
            self.h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params):
        self.params = copy_params(params)
        self._chk(self.lib.iba_set_params(self.h, C.byref(self.params)))

    @staticmethod
    def _x(x):
        x = np.ascontiguousarray(np.atleast_2d(x), np.float64)
        assert x.shape[1] == 7
        return x

    def eval_cost(self, x):
        x = self._x(x)
        B = len(x)
        out = (IbaCostOut * B)()
        self._chk(self.lib.iba_eval_cost(self.h, _p(x), C.c_int32(B), out))
        return list(out)

    def eval_bbo(self, x, he_threshold, valid_rate):
        x = self._x(x)
        B = len(x)
        out = (IbaBbo * B)()
        self._chk(self.lib.iba_eval_bbo(self.h, _p(x), C.c_int32(B), C.c_double(he_threshold), C.c_double(valid_rate), out))
        return list(out)

    def eval_normal(self, x):
        x = self._x(x)
        B = len(x)
        out = (IbaNormalOut * B)()
        self._chk(self.lib.iba_eval_normal(self.h, _p(x), C.c_int32(B), out))
        return list(out)

    def eval_full(self, x):
        x = self._x(x)
        B = len(x)
        cost = (IbaCostOut * B)()
        nrm = (IbaNormalOut * B)()
        self._chk(self.lib.iba_eval_full(self.h, _p(x), C.c_int32(B), cost, nrm))
        return list(cost), list(nrm)

    def calibrate_lm(self, x0, **opts):
        """iba_local's outer loop (re-associate, LM on the frozen problem, until allClose) on the device path."""
        o = IbaLmOptions()
        self.lib.iba_default_lm_options(C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        r = IbaLmResult()
        x0 = np.ascontiguousarray(x0, np.float64)
        self._chk(self.lib.iba_calibrate_lm(self.h, _p(x0), C.byref(o), C.byref(r)))
        return np.array(r.x[:]), r

    def calibrate_mads(self, x0, trace=False, record=False, **opts):
        """Global stage: batch-aware MADS on BALoss::eval_x's objective + 3 progressive-barrier constraints
        (the caller the reference gets from NOMAD, iba_global.cpp:551-602). opts override iba_default_mads_options;
        lb/ub given as 7-vectors are ABSOLUTE bounds. trace=True also returns the evaluated points (rows of x[7], f);
        record=True returns them together with the size of every black-box call (the batches iba_eval_bbo was given)."""
        x0 = np.ascontiguousarray(x0, np.float64)
        o = mads_options(x0, **opts)
        r = IbaMadsResult()
        if not trace and not record:
            self._chk(self.lib.iba_calibrate_mads(self.h, _p(x0), C.byref(o), C.byref(r)))
            return np.array(r.x[:]), r
        tr = np.zeros((int(o.max_bb_eval) + IBA_MAX_BATCH, 8))   # (the last batch may overshoot the budget by less than one batch)
        n = C.c_int32(0)
        if not record:
            self._chk(self.lib.iba_calibrate_mads_trace(self.h, _p(x0), C.byref(o), C.byref(r), _p(tr), C.c_int32(len(tr)), C.byref(n)))
            return np.array(r.x[:]), r, tr[: min(n.value, len(tr))]
        bs = np.zeros(len(tr), np.int32)
        nb = C.c_int32(0)
        self._chk(self.lib.iba_calibrate_mads_record(self.h, _p(x0), C.byref(o), C.byref(r), _p(tr), C.c_int32(len(tr)), C.byref(n), _p(bs), C.c_int32(len(bs)), C.byref(nb)))
        return np.array(r.x[:]), r, tr[: min(n.value, len(tr))], bs[: min(nb.value, len(bs))].copy()

    def build_problem(self, x):
        x = np.ascontiguousarray(x, np.float64)
        self._chk(self.lib.iba_build_problem(self.h, _p(x)))

    def eval_factors(self, x):
        x = self._x(x)
        B = len(x)
        out = (IbaNormalOut * B)()
        self._chk(self.lib.iba_eval_factors(self.h, _p(x), C.c_int32(B), out))
        return list(out)

    def eval_residuals(self, x):
        x = np.ascontiguousarray(x, np.float64)
        n = C.c_int64(0)
        self._chk(self.lib.iba_eval_residuals(self.h, _p(x), None, None, None, None, C.byref(n)))
        m = n.value
        r = np.zeros(m)
        J = np.zeros((m, 7))
        bid = np.zeros(m, np.int32)
        kind = np.zeros(m, np.int32)
        if m:
            self._chk(self.lib.iba_eval_residuals(self.h, _p(x), _p(r), _p(J), _p(bid), _p(kind), C.byref(n)))
        return r, J, bid, kind

    def correspondences(self, x, frame):
        o = self.problem.arrays["kp_offset"]
        K = int(o[frame + 1] - o[frame])
        kp = np.zeros(max(K, 1), np.uint32)
        pt = np.zeros(max(K, 1), np.uint32)
        n = C.c_int32(0)
        x = np.ascontiguousarray(x, np.float64)
        self._chk(self.lib.iba_get_correspondences(self.h, _p(x), C.c_int32(frame), _p(kp), _p(pt), C.c_int32(K), C.byref(n)))
        return kp[: n.value].copy(), pt[: n.value].copy()

    # --- multi-GPU building blocks: partial sums into caller-owned device memory ---
    def debug_nn(self, frame, queries, mode=1):
        """Exact 1-NN of LiDAR-frame query points in the scan of a (local) frame through the search kernel's own kd search
        (mode 1: as the association path's query, 2: as the cost path's, 3 / 4: both paths together, the query first / second):
        (original point indices, exact squared distances)."""
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, 3)
        idx = np.zeros(len(q), np.uint32)
        d2 = np.zeros(len(q), np.float64)
        self._chk(self.lib.iba_debug_nn(self.h, C.c_int32(frame), _p(q), C.c_int32(len(q)), C.c_int32(mode),
                                        idx.ctypes.data_as(C.POINTER(C.c_uint32)), _p(d2)))
        return idx, d2

    def call_latency(self, xs, kind="cost", iters=200):
        """(median_ms, min_ms) of a blocking entry point called `iters` times back to back from C (iba_debug_call_latency): kind = "cost"
        (iba_eval_cost), "full" (iba_eval_full) or "factors" (iba_eval_factors)"""
        xs = np.ascontiguousarray(xs, np.float64).reshape(-1, 7)
        med, mn = C.c_double(0), C.c_double(0)
        self.lib.iba_debug_call_latency.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        self._chk(self.lib.iba_debug_call_latency(self.h, _p(xs), C.c_int32(len(xs)), C.c_int32({"cost": 0, "full": 1, "factors": 2}[kind]), C.c_int32(iters), C.byref(med), C.byref(mn)))
        return med.value, mn.value

    def debug_knn(self, frame, points, k=30, r2=np.inf):
        """The sorted neighbour lists the plane fits build (iba_plane_kernel's list builder) around scan points given by ORIGINAL
        index: (idx [n, k], d2 [n, k], cnt [n])."""
        pts = np.ascontiguousarray(points, np.uint32).reshape(-1)
        n = len(pts)
        idx = np.zeros((n, k), np.uint32)
        d2 = np.zeros((n, k), np.float64)
        cnt = np.zeros(n, np.int32)
        self.lib.iba_debug_knn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.iba_debug_knn(self.h, C.c_int32(frame), _p(pts), C.c_int32(n), C.c_int32(k), C.c_double(r2), _p(idx), _p(d2), _p(cnt)))
        return idx, d2, cnt

    def debug_plane(self, frame, point, which=1):
        """(normal[3], reg_sum, far_d2, k) of the memoised local plane at ORIGINAL scan point index `point` of `frame` (which: 0 cost path, 1 local)"""
        out = np.zeros(5)
        k = C.c_int32(0)
        self._chk(self.lib.iba_debug_plane(self.h, C.c_int32(frame), C.c_uint32(int(point)), C.c_int32(which), _p(out), C.byref(k)))
        return out[:3].copy(), float(out[3]), float(out[4]), k.value

    def eval_cost_partial(self, x, d_partials_ptr, stream_ptr=None):
        x = self._x(x)
        self._chk(self.lib.iba_eval_cost_partial(self.h, _p(x), C.c_int32(len(x)), C.c_void_p(d_partials_ptr), C.c_void_p(stream_ptr)))

    def eval_normal_partial(self, x, d_partials_ptr, stream_ptr=None):
        x = self._x(x)
        self._chk(self.lib.iba_eval_normal_partial(self.h, _p(x), C.c_int32(len(x)), C.c_void_p(d_partials_ptr), C.c_void_p(stream_ptr)))

    @property
    def last_assoc2_threads(self):
        self.lib.iba_debug_last_assoc2_threads.argtypes = [C.c_void_p]
        self.lib.iba_debug_last_assoc2_threads.restype = C.c_int32
        return int(self.lib.iba_debug_last_assoc2_threads(self.h))

    def geo_correspondences(self, frame, src_xyz, max_distance=0.05):
        """GeoCalib.h:18-33 computeCorrespondence with the scan of local keyframe `frame` as the target cloud -> (source indices, target indices)"""
        src = np.ascontiguousarray(np.asarray(src_xyz, np.float64).reshape(-1, 3))
        n = len(src)
        o_s = np.zeros(max(n, 1), np.uint32); o_t = np.zeros(max(n, 1), np.uint32); cnt = C.c_int32(0)
        self.lib.iba_geo_correspondences.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        self._chk(self.lib.iba_geo_correspondences(self.h, C.c_int32(frame), _p(src), C.c_int32(n), C.c_double(max_distance), _p(o_s), _p(o_t), C.byref(cnt)))
        return o_s[: cnt.value].copy(), o_t[: cnt.value].copy()

    def icp_options(self, **fields):
        o = IbaIcpOptions()
        self._chk(self.lib.iba_default_icp_options(C.byref(o)))
        for k, v in fields.items():
            setattr(o, k, v)
        return o

    def icp_step(self, src_xyz, T, max_corr_dist, frames=(0, 1), pairs=False):
        """iba_icp_step: one correspondence pass per transform against the scans of local frames [frames[0], frames[1]) read as tiles of one cloud
        -> moments [B, ICP_NMOM] (layout: include/iba_mi355x.h), and with pairs=True (pair_frame, pair_idx) [B, n] (0xFFFFFFFF: not kept)"""
        src = np.ascontiguousarray(np.asarray(src_xyz, np.float64).reshape(-1, 3))
        T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1, 16))
        n, B = len(src), len(T)
        mom = np.zeros((B, ICP_NMOM))
        pf = np.zeros((B, max(n, 1)), np.uint32) if pairs else None
        pi = np.zeros((B, max(n, 1)), np.uint32) if pairs else None
        self.lib.iba_icp_step.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.lib.iba_icp_step(self.h, C.c_int32(frames[0]), C.c_int32(frames[1]), _p(src) if n else None, C.c_int32(n), _p(T), C.c_int32(B), C.c_double(max_corr_dist),
                                        _p(mom), _p(pf) if pairs else None, _p(pi) if pairs else None))
        return (mom, pf[:, :n], pi[:, :n]) if pairs else mom

    def icp_register(self, src_xyz, T_init, frames=(0, 1), **opts):
        """iba_icp_register: Open3D's RegistrationICP (point-to-point, with_scaling) from B independent starts -> list of IbaIcpResult"""
        src = np.ascontiguousarray(np.asarray(src_xyz, np.float64).reshape(-1, 3))
        T = np.ascontiguousarray(np.asarray(T_init, np.float64).reshape(-1, 16))
        n, B = len(src), len(T)
        o = self.icp_options(**opts)
        out = (IbaIcpResult * B)()
        self.lib.iba_icp_register.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(IbaIcpOptions), C.POINTER(IbaIcpResult)]
        self._chk(self.lib.iba_icp_register(self.h, C.c_int32(frames[0]), C.c_int32(frames[1]), _p(src) if n else None, C.c_int32(n), _p(T), C.c_int32(B), C.byref(o), out))
        return list(out)

    def icp_calib(self, cam_xyz, rigid12_init, scale_init, ref_lidar_pose12=None, frames=(0, 1), **opts):
        """iba_icp_calib: icp_calib.cpp:43-71 around the loop -> (rigid12 [3, 4], scale, IbaIcpResult) in readSim3 / writeSim3 form"""
        src = np.ascontiguousarray(np.asarray(cam_xyz, np.float64).reshape(-1, 3))
        r0 = np.ascontiguousarray(np.asarray(rigid12_init, np.float64).reshape(12))
        ref = None if ref_lidar_pose12 is None else np.ascontiguousarray(np.asarray(ref_lidar_pose12, np.float64).reshape(12))
        o = self.icp_options(**opts)
        out12 = np.zeros(12); sc = C.c_double(0.0); res = IbaIcpResult()
        self.lib.iba_icp_calib.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.POINTER(IbaIcpOptions), C.c_void_p,
                                           C.POINTER(C.c_double), C.POINTER(IbaIcpResult)]
        self._chk(self.lib.iba_icp_calib(self.h, C.c_int32(frames[0]), C.c_int32(frames[1]), _p(src) if len(src) else None, C.c_int32(len(src)), _p(r0), C.c_double(scale_init),
                                         None if ref is None else _p(ref), C.byref(o), _p(out12), C.byref(sc), C.byref(res)))
        return out12.reshape(3, 4), sc.value, res

    # --- scan-to-scan edges (iba_scan_*): a batch of (source frame, target frame, start) evaluated together ---
    @staticmethod
    def _edges(edges):
        """edges: iterable of (src_frame, tgt_frame, T 4x4) -> ctypes array of IbaScanEdge"""
        edges = list(edges)
        arr = (IbaScanEdge * max(len(edges), 1))()
        for k, (s, t, T) in enumerate(edges):
            arr[k].src_frame, arr[k].tgt_frame = int(s), int(t)
            arr[k].T[:] = np.asarray(T, np.float64).reshape(16).tolist()
        return arr, len(edges)

    def _scan_src_sizes(self, edges):
        o = self.problem.arrays["pt_offset"]
        return [int(o[self.frame_begin + int(s) + 1] - o[self.frame_begin + int(s)]) for s, _, _ in edges]

    def scan_step(self, edges, max_corr_dist, estimation=0, pairs=False):
        """iba_scan_step: one correspondence pass per edge -> sums [E, SCAN_NMOM] (layout: include/iba_mi355x.h), and with pairs=True a list of E
        uint32 arrays: per source point in ORIGINAL order the original index of its target point (0xFFFFFFFF: not kept)"""
        edges = list(edges)
        arr, E = self._edges(edges)
        mom = np.zeros((max(E, 1), SCAN_NMOM))
        sizes = self._scan_src_sizes(edges) if pairs else []
        pi = np.zeros(max(sum(sizes), 1), np.uint32) if pairs else None
        self.lib.iba_scan_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
        self._chk(self.lib.iba_scan_step(self.h, arr, C.c_int32(E), C.c_double(max_corr_dist), C.c_int32(estimation), _p(mom), _p(pi) if pairs else None))
        if not pairs:
            return mom[:E]
        cuts = np.cumsum([0] + sizes)
        return mom[:E], [pi[cuts[k]:cuts[k + 1]].copy() for k in range(E)]

    def scan_options(self, **fields):
        o = IbaScanOptions()
        self._chk(self.lib.iba_default_scan_options(C.byref(o)))
        for k, v in fields.items():
            if k not in dict(IbaScanOptions._fields_):
                raise AttributeError(k)
            setattr(o, k, v)
        return o

    def scan_register(self, edges, **opts):
        """iba_scan_register: RegistrationICP per edge (estimation 0 point-to-point, 1 point-to-plane; one stage or coarse -> refine), all edges
        together -> list of IbaScanResult"""
        arr, E = self._edges(edges)
        o = self.scan_options(**opts)
        out = (IbaScanResult * max(E, 1))()
        self.lib.iba_scan_register.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(IbaScanOptions), C.POINTER(IbaScanResult)]
        self._chk(self.lib.iba_scan_register(self.h, arr, C.c_int32(E), C.byref(o), out))
        return list(out)[:E]

    def scan_information(self, edges, max_dist):
        """iba_scan_information: GetInformationMatrixFromPointClouds per edge at its T -> (info [E, 6, 6], n_pairs [E])"""
        arr, E = self._edges(edges)
        info = np.zeros((max(E, 1), 36)); n = np.zeros(max(E, 1), np.int32)
        self.lib.iba_scan_information.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
        self._chk(self.lib.iba_scan_information(self.h, arr, C.c_int32(E), C.c_double(max_dist), _p(info), _p(n)))
        return info[:E].reshape(E, 6, 6), n[:E]

    # --- voxel down-sampling and merged sub-map clouds (iba_submap_build) ---
    def submap_build(self, subs):
        """iba_submap_build: subs = iterable of (frames, poses, out, voxel) — local frames [n], poses [n, 3, 4] (or [n, 12] / 4x4 each; scan frame ->
        common frame), out = None or a 3x4 / 4x4 applied to the averaged points, voxel size. -> list of dict(xyz [V, 3] float64 in ascending
        (ix, iy, iz), count [V] int32, n_dropped) per sub-map. LoadPCD of frame f: ([f], [np.eye(4)], None, voxel)."""
        arr, M, _keep = self._submap_descs(subs)
        return self.submap_build_raw(arr, M)

    @staticmethod
    def _submap_descs(subs):
        """-> (ctypes array of IbaSubmapDesc, M, the numpy arrays its pointers refer to)"""
        subs = list(subs)
        M = len(subs)
        arr = (IbaSubmapDesc * max(M, 1))()
        keep = []
        for k, (frames, poses, out, voxel) in enumerate(subs):
            fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
            ps = np.asarray(poses, np.float64)
            ps = np.ascontiguousarray(ps.reshape(len(fr), -1, 4)[:, :3, :] if len(fr) and ps.size == 16 * len(fr) else ps.reshape(len(fr), 12)).reshape(-1)
            o12 = None if out is None else np.ascontiguousarray(np.asarray(out, np.float64).reshape(-1, 4)[:3]).reshape(-1)
            keep.append((fr, ps, o12))
            arr[k].struct_size = C.sizeof(IbaSubmapDesc); arr[k].n_members = len(fr)
            arr[k].frames = fr.ctypes.data if len(fr) else None; arr[k].poses12 = ps.ctypes.data if len(fr) else None
            arr[k].out12 = None if o12 is None else o12.ctypes.data
            arr[k].voxel = float(voxel)
        return arr, M, keep

    def submap_build_raw(self, arr, M):
        """iba_submap_build on a ctypes array of IbaSubmapDesc (what submap_build fills)"""
        L = self.lib
        L.iba_submap_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        L.iba_submap_num.argtypes = [C.c_void_p]; L.iba_submap_num.restype = C.c_int32
        for f, rt in ((L.iba_submap_n_voxels, C.c_int64), (L.iba_submap_n_dropped, C.c_int64), (L.iba_submap_xyz, C.POINTER(C.c_double)), (L.iba_submap_counts, C.POINTER(C.c_int32))):
            f.argtypes = [C.c_void_p, C.c_int32]; f.restype = rt
        L.iba_submap_free.argtypes = [C.c_void_p]; L.iba_submap_free.restype = None
        res = C.c_void_p(None)
        self._chk(L.iba_submap_build(self.h, arr, C.c_int32(M), C.byref(res)))
        try:
            out = []
            for s in range(L.iba_submap_num(res)):
                V = int(L.iba_submap_n_voxels(res, s))
                xyz = np.ctypeslib.as_array(L.iba_submap_xyz(res, s), shape=(V, 3)).copy() if V else np.zeros((0, 3))
                cnt = np.ctypeslib.as_array(L.iba_submap_counts(res, s), shape=(V,)).copy() if V else np.zeros(0, np.int32)
                out.append(dict(xyz=xyz, count=cnt, n_dropped=int(L.iba_submap_n_dropped(res, s))))
        finally:
            L.iba_submap_free(res)
        return out

    # --- voxel clouds as the frames of a new handle, built on the device (iba_submap_handle) ---
    def submap_handle(self, subs, params=None):
        """iba_submap_handle: subs as for submap_build -> an IbaHandle whose local frame s is the voxel cloud of sub-map s (float32, voxel order),
        with the kd index built on the device. params: None = this handle's. The new handle does not depend on this one; close() it."""
        arr, M, _keep = self._submap_descs(subs)
        return self.submap_handle_raw(arr, M, params)

    def submap_handle_raw(self, arr, M, params=None):
        """iba_submap_handle on a ctypes array of IbaSubmapDesc"""
        L = self.lib
        L.iba_submap_handle.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(IbaParams), C.POINTER(C.c_void_p)]
        prm = copy_params(params if params is not None else self.params)
        out = C.c_void_p(None)
        self._chk(L.iba_submap_handle(self.h, arr, C.c_int32(M), C.byref(prm), C.byref(out)))
        return IbaHandle._adopt(L, out, prm, M)

    @classmethod
    def _adopt(cls, lib, h, params, n_frames):
        """wrap a handle the library created itself (scans only: the point counts are asked from the library)"""
        self = cls.__new__(cls)
        self.lib, self.h, self.params = lib, h, params
        self.frame_begin, self.frame_end = 0, n_frames
        counts = [self.frame_num_points(f) for f in range(n_frames)]
        self.problem = _ScanCounts(np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64))
        return self

    def frame_num_points(self, frame):
        self.lib.iba_frame_num_points.argtypes = [C.c_void_p, C.c_int32]
        self.lib.iba_frame_num_points.restype = C.c_int64
        return int(self.lib.iba_frame_num_points(self.h, C.c_int32(frame)))

    def debug_scan_index(self, frame):
        """iba_debug_scan_index: dict(perm [P] u32, xyz_tree [3, P] f32, node_dim / node_split [(1 << depth) - 1], chunk_box [chunks, 8] f32, frame_box [8] f32, depth)"""
        P = self.frame_num_points(frame)
        depth = C.c_int32(0)
        self.lib.iba_debug_scan_index.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.POINTER(C.c_int32)]
        self._chk(self.lib.iba_debug_scan_index(self.h, C.c_int32(frame), None, None, None, None, None, None, C.byref(depth)))
        nn, nc = (1 << depth.value) - 1, (P + 63) // 64
        r = dict(perm=np.zeros(P, np.uint32), xyz_tree=np.zeros((3, P), np.float32), node_dim=np.zeros(nn, np.uint32), node_split=np.zeros(nn, np.float32),
                 chunk_box=np.zeros((nc, 8), np.float32), frame_box=np.zeros(8, np.float32))
        self._chk(self.lib.iba_debug_scan_index(self.h, C.c_int32(frame), _p(r["perm"]), _p(r["xyz_tree"]), _p(r["node_dim"]), _p(r["node_split"]), _p(r["chunk_box"]), _p(r["frame_box"]), C.byref(depth)))
        r["depth"] = depth.value
        return r

    # --- Scan Context (iba_sc_describe): descriptors of resident scans as a database on the device ---
    def sc_describe(self, frames, opt=None, **fields):
        """iba_sc_describe: local frames [n] -> ScDb (nodes 0 .. n - 1). opt = an IbaScOptions, or fields of one over the reference's defaults."""
        o = sc_options(**fields) if opt is None else opt
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        self.lib.iba_sc_describe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
        db = C.c_void_p(None)
        self._chk(self.lib.iba_sc_describe(self.h, _p(fr) if len(fr) else None, C.c_int32(len(fr)), C.byref(o), C.byref(db)))
        return ScDb(self.lib, db, o)

    # --- F-LOAM feature extraction (iba_floam_extract): the edge and surf clouds of resident scans ---
    def floam_extract(self, frames, opt=None, **fields):
        """iba_floam_extract: local frames [n] -> list of dict(edge_xyz, edge_index, surf_xyz, surf_index, n_nonfinite, n_out_of_range, n_no_ring,
        ring_points) per scan (floam.py). opt = an IbaFloamOptions, or fields of one over the reference's defaults."""
        from . import floam
        return floam.extract(self, frames, opt, **fields)

    # --- F-LOAM scan-to-map (iba_floam_map_*): edge / surf factors and registration against map clouds that are frames of this handle ---
    def floam_map_step(self, pairs, opt=None, nn=False, records=False, **fields):
        """iba_floam_map_step: [(src_edge_frame, src_surf_frame, map_edge_frame, map_surf_frame, T)] -> moments [B, floam_map.NMOM] (+ nn_idx / records
        per pair when asked; floam_map.py)"""
        from . import floam_map
        return floam_map.step(self, pairs, opt, nn, records, **fields)

    def floam_map_register(self, pairs, opt=None, **fields):
        """iba_floam_map_register: the same pairs -> list of dict(T, initial_cost, final_cost, passes, iterations, evaluations, n_edge, n_surf, status)"""
        from . import floam_map
        return floam_map.register(self, pairs, opt, **fields)

    # --- the lattice voxel filter with a crop box (iba_lattice_build): PCL's VoxelGrid + CropBox of F-LOAM's local map ---
    def lattice_build(self, subs):
        """iba_lattice_build: subs = iterable of (frames, poses, out, leaf, crop) — as for submap_build, crop = None or (lo [3], hi [3]) in the common
        frame -> list of dict(xyz [V, 3] float64 in ascending (ix, iy, iz), count [V] int32, n_dropped, n_cropped) per sub-map (floam_odom.py)"""
        from . import floam_odom
        return floam_odom.lattice_build(self, subs)

    # --- F-LOAM odometry (iba_floam_odom_run): extract, down-sample, solve against the local map and update it, a batch of tracks in lock-step ---
    def floam_odom(self, tracks, opt=None, **fields):
        """iba_floam_odom_run: tracks = [(frames [n] in time order, T0 4x4)] -> per track a list of dict per scan (floam_odom.odom). opt = an
        IbaFloamOdomOptions, or fields of one (extract = {...}, map = {...} for the nested blocks) over the reference's defaults."""
        from . import floam_odom
        return floam_odom.odom(self, tracks, opt, **fields)

    def debug_scan_threads(self, threads):
        """force the block shape of the scan pass kernel (64 / 256; 0: the rule)"""
        self.lib.iba_debug_scan_threads.argtypes = [C.c_void_p, C.c_int32]
        self._chk(self.lib.iba_debug_scan_threads(self.h, C.c_int32(threads)))

    @property
    def last_scan_threads(self):
        self.lib.iba_debug_last_scan_threads.argtypes = [C.c_void_p]
        self.lib.iba_debug_last_scan_threads.restype = C.c_int32
        return int(self.lib.iba_debug_last_scan_threads(self.h))

    def debug_factor_ranges(self, B):
        """ranges per candidate iba_factor2_kernel would cut a batch of B into; 0 = the default factor kernel runs"""
        self.lib.iba_debug_factor_ranges.argtypes = [C.c_void_p, C.c_int32]
        self.lib.iba_debug_factor_ranges.restype = C.c_int32
        return int(self.lib.iba_debug_factor_ranges(self.h, C.c_int32(B)))

    @property
    def last_nn_threads(self):
        """threads per block of the last search launch (64: one-wave blocks; 256)"""
        self.lib.iba_debug_last_nn_threads.argtypes = [C.c_void_p]
        self.lib.iba_debug_last_nn_threads.restype = C.c_int32
        return int(self.lib.iba_debug_last_nn_threads(self.h))

    @property
    def last_nn_list(self):
        """> 0: the last search launch was iba_nn_list_kernel (opt-in, IBA_NN_LIST=1) with that many workers per (XCD, group of candidates)"""
        self.lib.iba_debug_last_nn_list.argtypes = [C.c_void_p]
        self.lib.iba_debug_last_nn_list.restype = C.c_int32
        return int(self.lib.iba_debug_last_nn_list(self.h))

    def debug_last_partials(self, B):
        out = np.zeros((B, partial_stride()))
        self._chk(self.lib.iba_debug_last_partials(self.h, _p(out), C.c_int32(B)))
        return out

    def eval_full_partial(self, x, d_partials_ptr, stream_ptr=None):
        x = self._x(x)
        self._chk(self.lib.iba_eval_full_partial(self.h, _p(x), C.c_int32(len(x)), C.c_void_p(d_partials_ptr), C.c_void_p(stream_ptr)))

    @property
    def last_path(self):
        """1: the last evaluation shared the 2d-3d pair search over the batch, 0: every candidate searched for itself"""
        self.lib.iba_debug_last_path.argtypes = [C.c_void_p]
        return int(self.lib.iba_debug_last_path(self.h))

    @property
    def pairs_builds(self):
        self.lib.iba_debug_pairs_builds.argtypes = [C.c_void_p]
        return int(self.lib.iba_debug_pairs_builds(self.h))

    @property
    def pairs_visible(self):
        """(items in the pair search's visible-chunk list — 0: none ready —, rebuilds so far, 1 if the last pair search walked the list, items a full grid has)"""
        out = (C.c_int32 * 4)()
        self.lib.iba_debug_pairs_visible.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        self._chk(self.lib.iba_debug_pairs_visible(self.h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def pairs_chunks_passing(self, group=0):
        """chunks that pass the pair search's chunk test under the bound of a group of the last pair search (-1: none ran)"""
        self.lib.iba_debug_pairs_chunks_passing.restype = C.c_int64
        self.lib.iba_debug_pairs_chunks_passing.argtypes = [C.c_void_p, C.c_int32]
        return int(self.lib.iba_debug_pairs_chunks_passing(self.h, int(group)))

    def rescans(self, reset=True):
        """association blocks since the last reset that took the rescan-every-point fallback (speed only)"""
        self.lib.iba_debug_rescans.restype = C.c_int64
        self.lib.iba_debug_rescans.argtypes = [C.c_void_p, C.c_int32]
        return int(self.lib.iba_debug_rescans(self.h, 1 if reset else 0))

    def counters(self, reset=True):
        """(association blocks that rescanned every point, assoc2 blocks whose winner note list overflowed, 0, 0) since the last reset"""
        out = (C.c_uint32 * 4)()
        self.lib.iba_debug_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int32]
        self._chk(self.lib.iba_debug_counters(self.h, out, 1 if reset else 0))
        return tuple(int(v) for v in out)

    @property
    def pair_lists(self):
        """(overflowed pair lists, pair lists read, longest list) of the last call"""
        out = (C.c_int32 * 3)()
        self.lib.iba_debug_pair_lists.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        self._chk(self.lib.iba_debug_pair_lists(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def pair_list(self, frame, slot=-1):
        """the (original scan point index, keypoint id) pairs of one (list slot, frame) pair list of the last pair search, as an
        (n, 2) uint32 array in list order (slot -1: the slot of the last call's first group)"""
        self.lib.iba_debug_pair_list.restype = C.c_int32
        self.lib.iba_debug_pair_list.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        n = int(self.lib.iba_debug_pair_list(self.h, int(slot), int(frame), None, 0))
        if n < 0:
            raise ValueError("iba_debug_pair_list: bad slot or frame")
        out = np.zeros((max(n, 1), 2), dtype=np.uint32)
        n2 = int(self.lib.iba_debug_pair_list(self.h, int(slot), int(frame), out.ctypes.data, n))
        if n2 != n:
            raise RuntimeError("iba_debug_pair_list: the list changed between the calls")
        return out[:n]

    @property
    def last_pairs_threads(self):
        """form of the last shared pair search: threads per block of the one-wave-per-chunk kernel (64, 256, 512), 0 for the block kernel"""
        self.lib.iba_debug_last_pairs_threads.restype = C.c_int32
        self.lib.iba_debug_last_pairs_threads.argtypes = [C.c_void_p]
        return int(self.lib.iba_debug_last_pairs_threads(self.h))

    @property
    def mean_pairs(self):
        self.lib.iba_debug_mean_pairs.restype = C.c_double
        self.lib.iba_debug_mean_pairs.argtypes = [C.c_void_p]
        return float(self.lib.iba_debug_mean_pairs(self.h))

    @property
    def nn_left_to_tree(self):
        self.lib.iba_debug_nn_left_to_tree.restype = C.c_double
        self.lib.iba_debug_nn_left_to_tree.argtypes = [C.c_void_p]
        return float(self.lib.iba_debug_nn_left_to_tree(self.h))

    @property
    def anchor_builds(self):
        self.lib.iba_debug_anchor_builds.argtypes = [C.c_void_p]
        return int(self.lib.iba_debug_anchor_builds(self.h))

    def set_timing(self, on=True):
        self._chk(self.lib.iba_set_timing(self.h, C.c_int32(1 if on else 0)))

    def last_kernel_ms(self):
        a = C.c_float(0)
        b = C.c_float(0)
        self._chk(self.lib.iba_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @property
    def n_points(self):
        return int(self.lib.iba_num_points(self.h))

    @property
    def n_keypoints(self):
        return int(self.lib.iba_num_keypoints(self.h))


class _ScanCounts:
    """what IbaHandle's wrappers read of a problem, for a handle whose scans never were on the host (IbaHandle.submap_handle)"""

    def __init__(self, pt_offset):
        self.n_frames = len(pt_offset) - 1
        self.arrays = dict(pt_offset=pt_offset, kp_offset=np.zeros(len(pt_offset), np.uint64))


def debug_build_tree(xyz):
    """iba_debug_build_tree (host only, no GPU): the host build of the kd index on [P, 3] float32 points -> dict(perm, node_dim, node_split, depth)"""
    L = load_library()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    P = len(pts)
    L.iba_debug_build_tree.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    depth = C.c_int32(0)
    st = L.iba_debug_build_tree(_p(pts), C.c_uint32(P), None, None, None, C.byref(depth))
    if st != 0:
        raise IbaError(st, "iba_debug_build_tree")
    nn = (1 << depth.value) - 1
    r = dict(perm=np.zeros(P, np.uint32), node_dim=np.zeros(nn, np.uint32), node_split=np.zeros(nn, np.float32), depth=depth.value)
    st = L.iba_debug_build_tree(_p(pts), C.c_uint32(P), _p(r["perm"]), _p(r["node_dim"]), _p(r["node_split"]), C.byref(depth))
    if st != 0:
        raise IbaError(st, "iba_debug_build_tree")
    return r


def sc_options(**fields):
    """iba_default_sc_options (the reference's Scancontext.h constants) with fields overridden"""
    o = IbaScOptions()
    st = load_library().iba_default_sc_options(C.byref(o))
    if st != 0:
        raise IbaError(st, "iba_default_sc_options")
    for k, v in fields.items():
        if k not in dict(IbaScOptions._fields_):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def sc_replay_plan(sizes_at_call, opt=None, **fields):
    """iba_sc_replay_plan (host only): the descriptors held at each detectLoopClosureID call -> db_end per call (0: the early return)"""
    L = load_library()
    o = sc_options(**fields) if opt is None else opt
    sizes = np.ascontiguousarray(sizes_at_call, np.int32).reshape(-1)
    out = np.zeros(max(len(sizes), 1), np.int32)
    L.iba_sc_replay_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_sc_last_error.argtypes = [C.c_void_p]; L.iba_sc_last_error.restype = C.c_char_p
    st = L.iba_sc_replay_plan(_p(sizes) if len(sizes) else None, C.c_int32(len(sizes)), C.byref(o), _p(out))
    if st != 0:
        raise IbaError(st, L.iba_sc_last_error(None).decode())
    return out[:len(sizes)]


class ScDb:
    """iba_sc_db wrapper: the Scan Context database of iba_sc_describe (on the device until close())"""

    def __init__(self, lib, db, opt):
        self.lib, self.db, self.opt = lib, db, opt
        L = lib
        L.iba_sc_last_error.argtypes = [C.c_void_p]; L.iba_sc_last_error.restype = C.c_char_p
        L.iba_sc_db_size.argtypes = [C.c_void_p]; L.iba_sc_db_size.restype = C.c_int32
        L.iba_sc_db_free.argtypes = [C.c_void_p]; L.iba_sc_db_free.restype = None
        L.iba_sc_db_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
        L.iba_sc_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.iba_sc_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]

    def _chk(self, st):
        if st != 0:
            raise IbaError(st, self.lib.iba_sc_last_error(self.db).decode())

    def __len__(self):
        return int(self.lib.iba_sc_db_size(self.db))

    def read(self, first=0, count=None):
        """iba_sc_db_read -> dict(desc [count, R, S], ring [count, R], ring_f float32, sector [count, S], skipped [count] int64)"""
        n = len(self) - first if count is None else count
        R, S = self.opt.num_ring, self.opt.num_sector
        m = max(n, 0)
        out = dict(desc=np.zeros((m, R, S)), ring=np.zeros((m, R)), ring_f=np.zeros((m, R), np.float32), sector=np.zeros((m, S)), skipped=np.zeros(m, np.int64))
        self._chk(self.lib.iba_sc_db_read(self.db, C.c_int32(first), C.c_int32(n), _p(out["desc"]), _p(out["ring"]), _p(out["ring_f"]), _p(out["sector"]), _p(out["skipped"])))
        return out

    def distance(self, pairs, opt=None):
        """iba_sc_distance: pairs [P, 2] of nodes -> (dist [P] float64, shift [P] int32)"""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        P = len(pr)
        dist, shift = np.zeros(max(P, 1)), np.zeros(max(P, 1), np.int32)
        self._chk(self.lib.iba_sc_distance(self.db, _p(pr) if P else None, C.c_int32(P), C.byref(opt or self.opt), _p(dist), _p(shift)))
        return dist[:P], shift[:P]

    def detect(self, queries, opt=None):
        """iba_sc_detect: queries = [(node, db_end)] -> ctypes array of IbaScResult"""
        qs = list(queries)
        Q = len(qs)
        arr = (IbaScQuery * max(Q, 1))()
        for i, (node, db_end) in enumerate(qs):
            arr[i].struct_size = C.sizeof(IbaScQuery); arr[i].node = int(node); arr[i].db_end = int(db_end)
        return self.detect_raw(arr, Q, opt)

    def detect_raw(self, arr, Q, opt=None):
        out = (IbaScResult * max(Q, 1))()
        self._chk(self.lib.iba_sc_detect(self.db, arr, C.c_int32(Q), C.byref(opt or self.opt), out))
        return out

    def close(self):
        if getattr(self, "db", None) and self.db.value:
            self.lib.iba_sc_db_free(self.db)
            self.db = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IbaGroup:
    """iba_group wrapper: one process, several GPUs of a node, frames sharded over them, one RCCL all-reduce per evaluation."""

    def __init__(self, problem, params=None, devices=(0,), host_reduce=False):
        """host_reduce: sum the partial blocks on the host in rank order (IBA_GROUP_REDUCE_HOST; no RCCL, a device may repeat)."""
        self.lib = load_library()
        self.problem = problem
        self.params = copy_params(params) if params is not None else default_params()
        self._desc = problem.desc()
        self.g = C.c_void_p(None)
        dev = (C.c_int32 * len(devices))(*devices)
        self.lib.iba_group_last_error.restype = C.c_char_p
        self.lib.iba_group_last_error.argtypes = [C.c_void_p]
        self.lib.iba_group_destroy.argtypes = [C.c_void_p]
        self.lib.iba_group_last_issue_us.restype = C.c_double
        self.lib.iba_group_last_issue_us.argtypes = [C.c_void_p]
        self.lib.iba_group_comm_ranks.argtypes = [C.c_void_p]
        st = self.lib.iba_group_create_ex(C.byref(self._desc), C.byref(self.params), dev, C.c_int32(len(devices)), C.c_int32(1 if host_reduce else 0), C.byref(self.g))
        if st != 0:
            raise IbaError(st, self.lib.iba_group_last_error(None).decode())

    @property
    def comm_ranks(self):
        """ncclCommCount of the group's communicator (0: host reduction)."""
        return int(self.lib.iba_group_comm_ranks(self.g))

    @property
    def last_issue_us(self):
        return float(self.lib.iba_group_last_issue_us(self.g))

    @property
    def last_enqueue_us(self):
        """host time until the last device's launch chain and collective of the last call were enqueued"""
        self.lib.iba_group_last_enqueue_us.restype = C.c_double
        self.lib.iba_group_last_enqueue_us.argtypes = [C.c_void_p]
        return float(self.lib.iba_group_last_enqueue_us(self.g))

    def set_params(self, params):
        self.params = copy_params(params)
        self._chk(self.lib.iba_group_set_params(self.g, C.byref(self.params)))

    def _chk(self, st):
        if st != 0:
            raise IbaError(st, self.lib.iba_group_last_error(self.g).decode())

    def close(self):
        if getattr(self, "g", None) and self.g.value:
            self.lib.iba_group_destroy(self.g)
            self.g = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frame_range(self, rank):
        a, b = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.iba_group_frame_range(self.g, C.c_int32(rank), C.byref(a), C.byref(b)))
        return a.value, b.value

    def eval_cost(self, x):
        x = IbaHandle._x(x)
        out = (IbaCostOut * len(x))()
        self._chk(self.lib.iba_group_eval_cost(self.g, _p(x), C.c_int32(len(x)), out))
        return list(out)

    def eval_full(self, x):
        x = IbaHandle._x(x)
        cost, nrm = (IbaCostOut * len(x))(), (IbaNormalOut * len(x))()
        self._chk(self.lib.iba_group_eval_full(self.g, _p(x), C.c_int32(len(x)), cost, nrm))
        return list(cost), list(nrm)

    def eval_normal(self, x):
        x = IbaHandle._x(x)
        nrm = (IbaNormalOut * len(x))()
        self._chk(self.lib.iba_group_eval_normal(self.g, _p(x), C.c_int32(len(x)), nrm))
        return list(nrm)

    def build_problem(self, x):
        x = np.ascontiguousarray(x, np.float64)
        self._chk(self.lib.iba_group_build_problem(self.g, _p(x)))

    def eval_factors(self, x):
        x = IbaHandle._x(x)
        nrm = (IbaNormalOut * len(x))()
        self._chk(self.lib.iba_group_eval_factors(self.g, _p(x), C.c_int32(len(x)), nrm))
        return list(nrm)

    def calibrate_lm(self, x0, **opts):
        o = IbaLmOptions()
        self.lib.iba_default_lm_options(C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        r = IbaLmResult()
        x0 = np.ascontiguousarray(x0, np.float64)
        self._chk(self.lib.iba_group_calibrate_lm(self.g, _p(x0), C.byref(o), C.byref(r)))
        return np.array(r.x[:]), r

    def calibrate_mads(self, x0, **opts):
        x0 = np.ascontiguousarray(x0, np.float64)
        o = mads_options(x0, **opts)
        r = IbaMadsResult()
        self._chk(self.lib.iba_group_calibrate_mads(self.g, _p(x0), C.byref(o), C.byref(r)))
        return np.array(r.x[:]), r


def rccl_info():
    """(text, runtime version code, header version code) of the librccl this process runs (loaded lazily by the library)."""
    L = load_library()
    buf = C.create_string_buffer(1024)
    rv, hv = C.c_int32(0), C.c_int32(0)
    st = L.iba_rccl_info(buf, C.c_int32(1024), C.byref(rv), C.byref(hv))
    if st != 0:
        raise IbaError(st, buf.value.decode())
    return buf.value.decode(), rv.value, hv.value


def mads_options(x0, **opts):
    L = load_library()
    x0 = np.ascontiguousarray(x0, np.float64)
    o = IbaMadsOptions()
    L.iba_default_mads_options(_p(x0), C.byref(o))
    for k, v in opts.items():
        if k in ("lb", "ub", "init_frame"):
            for i in range(7):
                getattr(o, k)[i] = float(v[i])
        else:
            setattr(o, k, v)
    return o


def debug_cand(x):
    """(host only) R[9], t[3], dR[3][9], dt[6][3], s of a candidate exactly as the factor kernel reads them: 58 doubles"""
    L = load_library()
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros(58)
    L.iba_debug_cand.argtypes = [C.c_void_p, C.c_void_p]
    st = L.iba_debug_cand(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise IbaError(st, "iba_debug_cand")
    return out


def debug_div2_selftest(num0, num1, den, device=0):
    """(q0, q1, ref0, ref1, n_fast): num0 / den and num1 / den as the kernels' shared-reciprocal division computes them, as the compiler's
    f64 division does, and how many triples took the shared-reciprocal path (include/iba_mi355x_debug.h)."""
    L = load_library()
    a, b, d = (np.ascontiguousarray(v, np.float64).reshape(-1) for v in (num0, num1, den))
    assert len(a) == len(b) == len(d)
    out = [np.zeros(len(a)) for _ in range(4)]
    nf = C.c_int64(0)
    L.iba_debug_div2_selftest.argtypes = [C.c_int32] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4 + [C.POINTER(C.c_int64)]
    st = L.iba_debug_div2_selftest(C.c_int32(device), _p(a), _p(b), _p(d), C.c_int64(len(a)), *[_p(o) for o in out], C.byref(nf))
    if st != 0:
        raise IbaError(st, "iba_debug_div2_selftest")
    return out[0], out[1], out[2], out[3], nf.value


def mads_selftest(problem, x0, trace=False, **opts):
    """The MADS driver on a built-in analytic black box (host only, no GPU). trace=True also returns the evaluated points."""
    L = load_library()
    x0 = np.ascontiguousarray(x0, np.float64)
    o = mads_options(x0, **opts)
    r = IbaMadsResult()
    tr = np.zeros((int(o.max_bb_eval) if trace else 1, 8))
    n = C.c_int32(0)
    st = L.iba_mads_selftest_trace(C.c_int32(problem), _p(x0), C.byref(o), C.byref(r), _p(tr) if trace else None, C.c_int32(len(tr) if trace else 0), C.byref(n))
    if st != 0:
        raise IbaError(st, "iba_mads_selftest")
    return (np.array(r.x[:]), r, tr[: n.value]) if trace else (np.array(r.x[:]), r)


def shard_frames(n_frames, world_size, rank, weights=None):
    """Contiguous frame range of `rank`, balanced by `weights` (points per frame; uniform if None)."""
    w = np.ones(n_frames) if weights is None else np.asarray(weights, np.float64)
    c = np.concatenate([[0.0], np.cumsum(w)])
    tot = c[-1]
    cuts = [int(np.searchsorted(c, tot * r / world_size, side="left")) for r in range(world_size + 1)]
    cuts[0], cuts[-1] = 0, n_frames
    for i in range(1, world_size + 1):
        cuts[i] = max(cuts[i], cuts[i - 1])
    return cuts[rank], cuts[rank + 1]
