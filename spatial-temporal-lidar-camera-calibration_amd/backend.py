"""ctypes mirror of the back end's loop-closure run (include/iba_mi355x.h, iba_backend_*; csrc/iba_backend.hip): the options of backend.yml, the plan —
keyframes, described frames, detection calls — which needs no device, and the run on a handle of raw scans. Plumbing only."""
import ctypes as C

import numpy as np

from . import IbaError, load_library
from .abi import IbaScanOptions, IbaScOptions
from .smooth import IbaSmoothOptions


class IbaBackendOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("lc_submap_size", C.c_int32), ("voxel", C.c_double), ("keyframe_meter_gap", C.c_double), ("keyframe_rad_gap", C.c_double),
                ("lc_keyframe_meter_gap", C.c_double), ("lc_keyframe_rad_gap", C.c_double), ("loop_overlap_thre", C.c_double), ("loop_inlier_rmse_thre", C.c_double),
                ("sc", IbaScOptions), ("scan", IbaScanOptions), ("prior_var", C.c_double * 6), ("odom_var", C.c_double * 6), ("loop_var", C.c_double * 6),
                ("smooth", IbaSmoothOptions), ("cloud_lag", C.c_int32), ("keep_update_poses", C.c_int32)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _lib():
    L = load_library()
    L.iba_backend_last_error.restype = C.c_char_p
    L.iba_backend_last_error.argtypes = []
    L.iba_default_backend_options.argtypes = [C.POINTER(IbaBackendOptions)]
    L.iba_backend_plan.argtypes = [C.c_void_p, C.c_int32, C.POINTER(IbaBackendOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32)]
    return L


def backend_options(**fields):
    """iba_default_backend_options (config/loam/backend.yml, BackEndOption) with fields overridden; sc_ / scan_ / smooth_ prefixes reach the embedded
    options, prior_var / odom_var / loop_var take six numbers"""
    o = IbaBackendOptions()
    st = _lib().iba_default_backend_options(C.byref(o))
    if st != 0:
        raise IbaError(st, "iba_default_backend_options")
    for k, v in fields.items():
        target, name = o, k
        for prefix in ("sc_", "scan_", "smooth_"):
            if k.startswith(prefix) and k[len(prefix):] in dict(getattr(o, prefix[:-1])._fields_):
                target, name = getattr(o, prefix[:-1]), k[len(prefix):]
        if name not in dict(type(target)._fields_):
            raise AttributeError(k)
        if name in ("prior_var", "odom_var", "loop_var"):
            getattr(target, name)[:] = [float(x) for x in np.asarray(v, np.float64).reshape(6)]
        else:
            setattr(target, name, v)
    return o


def backend_plan(poses12, opt=None, **fields):
    """iba_backend_plan (host only): poses [N, 12] or [N, 3, 4] -> dict(keyframes [K], described [K], detects [K] bool, sizes_at_call [C])"""
    L = _lib()
    o = backend_options(**fields) if opt is None else opt
    ps = np.ascontiguousarray(np.asarray(poses12, np.float64).reshape(-1, 12))
    N = len(ps)
    kf, ds, dt, sz = np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.uint8), np.zeros(max(N, 1), np.int32)
    nk, nc = C.c_int32(0), C.c_int32(0)
    st = L.iba_backend_plan(_p(ps) if N else None, C.c_int32(N), C.byref(o), _p(kf), _p(ds), _p(dt), C.byref(nk), _p(sz), C.byref(nc))
    if st != 0:
        raise IbaError(st, L.iba_backend_last_error().decode())
    return dict(keyframes=kf[:nk.value].copy(), described=ds[:nk.value].copy(), detects=dt[:nk.value].astype(bool), sizes_at_call=sz[:nc.value].copy())


class IbaBackendDetection(C.Structure):
    _fields_ = [("query_frame", C.c_int32), ("history_frame", C.c_int32), ("accepted", C.c_int32), ("reserved", C.c_int32), ("sc_dist", C.c_double),
                ("fitness", C.c_double), ("rmse", C.c_double), ("T", C.c_double * 16)]


def backend_run(handle, poses12, opt=None, **fields):
    """iba_backend_run on an IbaHandle whose frames 0 .. N - 1 are the raw scans: -> dict(poses [N, 3, 4], keyframes [K], detections [list of dict(query,
    history, sc_dist, fitness, rmse, T [4, 4], accepted)], updates [list of IbaSmoothResult], update_poses [per update [n_nodes, 3, 4], or None without
    keep_update_poses])"""
    from .smooth import IbaSmoothResult
    L = _lib()
    L.iba_backend_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(IbaBackendOptions), C.POINTER(C.c_void_p)]
    L.iba_backend_result_free.argtypes = [C.c_void_p]
    L.iba_backend_result_free.restype = None
    for name, rt in (("poses12", C.POINTER(C.c_double)), ("keyframes", C.POINTER(C.c_int32)), ("detections", C.POINTER(IbaBackendDetection)), ("updates", C.POINTER(IbaSmoothResult))):
        getattr(L, "iba_backend_result_" + name).argtypes = [C.c_void_p]
        getattr(L, "iba_backend_result_" + name).restype = rt
    for name in ("n_frames", "n_keyframes", "n_detections", "n_updates"):
        getattr(L, "iba_backend_result_" + name).argtypes = [C.c_void_p]
    o = backend_options(**fields) if opt is None else opt
    ps = np.ascontiguousarray(np.asarray(poses12, np.float64).reshape(-1, 12))
    r = C.c_void_p(None)
    st = L.iba_backend_run(handle.h, _p(ps) if len(ps) else None, C.c_int32(len(ps)), C.byref(o), C.byref(r))
    if st != 0:
        raise IbaError(st, L.iba_backend_last_error().decode())
    try:
        n, k, nd, nu = (getattr(L, "iba_backend_result_" + x)(r) for x in ("n_frames", "n_keyframes", "n_detections", "n_updates"))
        poses = np.ctypeslib.as_array(L.iba_backend_result_poses12(r), (n * 12,)).reshape(n, 3, 4).copy()
        keyframes = np.ctypeslib.as_array(L.iba_backend_result_keyframes(r), (k,)).copy()
        det = L.iba_backend_result_detections(r)
        detections = [dict(query=det[i].query_frame, history=det[i].history_frame, sc_dist=det[i].sc_dist, fitness=det[i].fitness, rmse=det[i].rmse,
                           T=np.array(det[i].T[:]).reshape(4, 4), accepted=bool(det[i].accepted)) for i in range(nd)]
        up = L.iba_backend_result_updates(r)
        L.iba_backend_result_update_poses12.argtypes = [C.c_void_p, C.c_int32]
        L.iba_backend_result_update_poses12.restype = C.POINTER(C.c_double)
        updates, update_poses = [], []
        for i in range(nu):
            u = IbaSmoothResult()
            C.memmove(C.byref(u), C.byref(up[i]), C.sizeof(u))
            updates.append(u)
            pp = L.iba_backend_result_update_poses12(r, i)
            update_poses.append(np.ctypeslib.as_array(pp, (u.n_nodes * 12,)).reshape(-1, 3, 4).copy() if pp else None)
    finally:
        L.iba_backend_result_free(r)
    return dict(poses=poses, keyframes=keyframes, detections=detections, updates=updates, update_poses=update_poses)
