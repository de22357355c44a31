"""ctypes mirror of the F-LOAM odometry block (include/iba_mi355x.h): the lattice voxel filter with a crop box (iba_lattice_build,
csrc/iba_voxel_host.hpp) — PCL's VoxelGrid and CropBox as the local map uses them — and the track loop (iba_floam_odom_run,
csrc/iba_floam_odom_host.hpp): a batch of tracks of resident scans in, a pose per scan out. Plumbing only."""
import ctypes as C

import numpy as np

from . import IbaError, load_library
from .abi import IbaFloamOptions
from .floam_map import IbaFloamMapOptions


class IbaLatticeDesc(C.Structure):
    """iba_lattice_desc: one sub-map of iba_lattice_build (members = local frames + poses, optional output transform, leaf, optional crop box)"""
    _fields_ = [("struct_size", C.c_int32), ("n_members", C.c_int32), ("frames", C.c_void_p), ("poses12", C.c_void_p), ("out12", C.c_void_p),
                ("leaf", C.c_double), ("has_crop", C.c_int32), ("reserved", C.c_int32), ("crop_lo", C.c_double * 3), ("crop_hi", C.c_double * 3)]


assert C.sizeof(IbaLatticeDesc) == 96


def _lib():
    L = load_library()
    L.iba_lattice_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.iba_submap_num.argtypes = [C.c_void_p]; L.iba_submap_num.restype = C.c_int32
    for f, rt in ((L.iba_submap_n_voxels, C.c_int64), (L.iba_submap_n_dropped, C.c_int64), (L.iba_submap_n_cropped, C.c_int64), (L.iba_submap_xyz, C.POINTER(C.c_double)),
                  (L.iba_submap_counts, C.POINTER(C.c_int32))):
        f.argtypes = [C.c_void_p, C.c_int32]; f.restype = rt
    L.iba_submap_free.argtypes = [C.c_void_p]; L.iba_submap_free.restype = None
    return L


def make_descs(subs):
    """[(frames, poses, out, leaf, crop)] — as IbaHandle.submap_build takes them, crop = None or (lo [3], hi [3]) in the common frame
    -> (ctypes array of IbaLatticeDesc, M, the numpy arrays its pointers refer to)"""
    subs = list(subs)
    M = len(subs)
    arr = (IbaLatticeDesc * max(M, 1))()
    keep = []
    for k, (frames, poses, out, leaf, crop) in enumerate(subs):
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        ps = np.asarray(poses, np.float64)
        ps = np.ascontiguousarray(ps.reshape(len(fr), -1, 4)[:, :3, :] if len(fr) and ps.size == 16 * len(fr) else ps.reshape(len(fr), 12)).reshape(-1)
        o12 = None if out is None else np.ascontiguousarray(np.asarray(out, np.float64).reshape(-1, 4)[:3]).reshape(-1)
        keep.append((fr, ps, o12))
        a = arr[k]
        a.struct_size = C.sizeof(IbaLatticeDesc); a.n_members = len(fr)
        a.frames = fr.ctypes.data if len(fr) else None; a.poses12 = ps.ctypes.data if len(fr) else None
        a.out12 = None if o12 is None else o12.ctypes.data
        a.leaf = float(leaf)
        a.has_crop = 0 if crop is None else 1
        if crop is not None:
            a.crop_lo[:] = [float(v) for v in np.asarray(crop[0], np.float64).reshape(3)]
            a.crop_hi[:] = [float(v) for v in np.asarray(crop[1], np.float64).reshape(3)]
    return arr, M, keep


def lattice_build_raw(handle, arr, M):
    """iba_lattice_build on a ctypes array of IbaLatticeDesc -> list of dict(xyz [V, 3] float64 in ascending (ix, iy, iz), count [V] int32, n_dropped,
    n_cropped) per sub-map"""
    L = _lib()
    res = C.c_void_p(None)
    handle._chk(L.iba_lattice_build(handle.h, arr, C.c_int32(M), C.byref(res)))
    try:
        out = []
        for s in range(L.iba_submap_num(res)):
            V = int(L.iba_submap_n_voxels(res, s))
            xyz = np.ctypeslib.as_array(L.iba_submap_xyz(res, s), shape=(V, 3)).copy() if V else np.zeros((0, 3))
            cnt = np.ctypeslib.as_array(L.iba_submap_counts(res, s), shape=(V,)).copy() if V else np.zeros(0, np.int32)
            out.append(dict(xyz=xyz, count=cnt, n_dropped=int(L.iba_submap_n_dropped(res, s)), n_cropped=int(L.iba_submap_n_cropped(res, s))))
    finally:
        L.iba_submap_free(res)
    return out


def lattice_build(handle, subs):
    """iba_lattice_build: subs as for make_descs"""
    arr, M, _keep = make_descs(subs)
    return lattice_build_raw(handle, arr, M)


# ---- the track loop ----
class IbaFloamTrack(C.Structure):
    """iba_floam_track"""
    _fields_ = [("n_scans", C.c_int32), ("frames", C.c_void_p), ("T0", C.c_double * 16)]


class IbaFloamOdomOptions(C.Structure):
    """iba_floam_odom_options (iba_default_floam_odom_options fills it, the nested blocks included)"""
    _fields_ = [("struct_size", C.c_int32), ("init_passes", C.c_int32), ("keep_maps", C.c_int32), ("reserved", C.c_int32), ("map_resolution", C.c_double),
                ("crop_half", C.c_double), ("extract", IbaFloamOptions), ("map", IbaFloamMapOptions)]


class IbaFloamOdomStep(C.Structure):
    """iba_floam_odom_step"""
    _fields_ = [("T_pred", C.c_double * 16), ("T", C.c_double * 16), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("passes", C.c_int32),
                ("iterations", C.c_int32), ("evaluations", C.c_int32), ("n_edge", C.c_int32), ("n_surf", C.c_int32), ("status", C.c_int32),
                ("n_src_edge", C.c_int64), ("n_src_surf", C.c_int64), ("n_map_edge", C.c_int64), ("n_map_surf", C.c_int64)]


def _odom_lib():
    L = load_library()
    L.iba_default_floam_odom_options.argtypes = [C.c_void_p]
    L.iba_floam_odom_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.iba_floam_odom_num.argtypes = [C.c_void_p]; L.iba_floam_odom_num.restype = C.c_int32
    L.iba_floam_odom_n_scans.argtypes = [C.c_void_p, C.c_int32]; L.iba_floam_odom_n_scans.restype = C.c_int32
    L.iba_floam_odom_steps.argtypes = [C.c_void_p, C.c_int32]; L.iba_floam_odom_steps.restype = C.POINTER(IbaFloamOdomStep)
    for f in (L.iba_floam_odom_src, L.iba_floam_odom_map):
        f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]; f.restype = C.POINTER(C.c_float)
    L.iba_floam_odom_free.argtypes = [C.c_void_p]; L.iba_floam_odom_free.restype = None
    return L


def odom_options(extract=None, map=None, **fields):
    """iba_default_floam_odom_options with fields overridden; extract / map: dicts of fields of the nested blocks"""
    o = IbaFloamOdomOptions()
    st = _odom_lib().iba_default_floam_odom_options(C.byref(o))
    if st != 0:
        raise IbaError(st, "iba_default_floam_odom_options")
    for k, v in fields.items():
        if k not in dict(IbaFloamOdomOptions._fields_) or k in ("extract", "map"):
            raise KeyError(k)
        setattr(o, k, v)
    for block, kw in ((o.extract, extract), (o.map, map)):
        for k, v in (kw or {}).items():
            if k not in dict(type(block)._fields_):
                raise KeyError(k)
            setattr(block, k, v)
    return o


def make_tracks(tracks):
    """[(frames [n], T0 4x4)] -> (array of iba_floam_track, the numpy arrays its pointers refer to)"""
    arr = (IbaFloamTrack * max(len(tracks), 1))()
    keep = []
    for a, (frames, T0) in zip(arr, tracks):
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        keep.append(fr)
        a.n_scans = len(fr); a.frames = fr.ctypes.data if len(fr) else None
        a.T0[:] = list(np.asarray(T0, np.float64).reshape(16))
    return arr, keep


def _cloud(fn, res, b, k, kind):
    n = C.c_int64(-1)
    p = fn(res, b, k, kind, C.byref(n))
    if n.value < 0:
        return None
    return np.ctypeslib.as_array(p, shape=(n.value, 3)).copy() if n.value else np.zeros((0, 3), np.float32)


def odom(handle, tracks, opt=None, **fields):
    """iba_floam_odom_run: tracks = [(frames [n], T0 4x4)] -> per track a list of dict per scan: T_pred, T [4, 4], initial_cost, final_cost, passes,
    iterations, evaluations, n_edge, n_surf, status, n_src_edge, n_src_surf, n_map_edge, n_map_surf, src_edge, src_surf [*, 3] float32 (the
    down-sampled clouds), map_edge, map_surf (the map after the step; None where it was not kept: every step but the last without keep_maps)"""
    L = _odom_lib()
    o = odom_options(**fields) if opt is None else opt
    arr, _keep = make_tracks(tracks)
    res = C.c_void_p(None)
    handle._chk(L.iba_floam_odom_run(handle.h, C.byref(arr), C.c_int32(len(tracks)), C.byref(o), C.byref(res)))
    try:
        out = []
        for b in range(L.iba_floam_odom_num(res)):
            steps = L.iba_floam_odom_steps(res, b)
            tr = []
            for k in range(L.iba_floam_odom_n_scans(res, b)):
                s = steps[k]
                d = dict(T_pred=np.array(s.T_pred[:]).reshape(4, 4), T=np.array(s.T[:]).reshape(4, 4))
                for name in ("initial_cost", "final_cost", "passes", "iterations", "evaluations", "n_edge", "n_surf", "status", "n_src_edge", "n_src_surf", "n_map_edge", "n_map_surf"):
                    d[name] = getattr(s, name)
                d["src_edge"] = _cloud(L.iba_floam_odom_src, res, b, k, 0); d["src_surf"] = _cloud(L.iba_floam_odom_src, res, b, k, 1)
                d["map_edge"] = _cloud(L.iba_floam_odom_map, res, b, k, 0); d["map_surf"] = _cloud(L.iba_floam_odom_map, res, b, k, 1)
                tr.append(d)
            out.append(tr)
    finally:
        L.iba_floam_odom_free(res)
    return out
