"""ctypes mirror of the F-LOAM scan-to-map block (include/iba_mi355x.h, iba_floam_map_*; csrc/iba_floam_map_host.hpp): edge / surf factors and the
registration of a batch of (scan clouds, map clouds, start pose) pairs whose clouds are frames of one handle. Plumbing only."""
import ctypes as C

import numpy as np

from . import IbaError, load_library

NMOM = 34            # IBA_FLOAM_NMOM
OK, DEGENERATE = 0, 1
NONE = 0xFFFFFFFF


class IbaFloamPair(C.Structure):
    """iba_floam_pair"""
    _fields_ = [("src_edge_frame", C.c_int32), ("src_surf_frame", C.c_int32), ("map_edge_frame", C.c_int32), ("map_surf_frame", C.c_int32), ("T", C.c_double * 16)]


class IbaFloamMapOptions(C.Structure):
    """iba_floam_map_options: the constants of the reference's odomEstimationClass.cpp (iba_default_floam_map_options fills them)"""
    _fields_ = [("struct_size", C.c_int32), ("k", C.c_int32), ("max_nn_dist2", C.c_double), ("edge_eig_ratio", C.c_double), ("edge_half_len", C.c_double),
                ("plane_max_resid", C.c_double), ("huber_delta", C.c_double), ("outer_passes", C.c_int32), ("inner_iterations", C.c_int32),
                ("min_map_edge", C.c_int32), ("min_map_surf", C.c_int32)]


class IbaFloamRecord(C.Structure):
    """iba_floam_record"""
    _fields_ = [("kind", C.c_int32), ("tried", C.c_int32), ("v", C.c_double * 7)]


class IbaFloamMapResult(C.Structure):
    """iba_floam_map_result"""
    _fields_ = [("T", C.c_double * 16), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("passes", C.c_int32), ("iterations", C.c_int32),
                ("evaluations", C.c_int32), ("n_edge", C.c_int32), ("n_surf", C.c_int32), ("status", C.c_int32)]


RECORD_DTYPE = np.dtype([("kind", np.int32), ("tried", np.int32), ("v", np.float64, (7,))])
assert RECORD_DTYPE.itemsize == C.sizeof(IbaFloamRecord) == 64


def _lib():
    L = load_library()
    L.iba_default_floam_map_options.argtypes = [C.c_void_p]
    L.iba_floam_map_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_floam_map_register.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    return L


def map_options(**fields):
    """iba_default_floam_map_options (the reference's constants) with fields overridden"""
    o = IbaFloamMapOptions()
    st = _lib().iba_default_floam_map_options(C.byref(o))
    if st != 0:
        raise IbaError(st, "iba_default_floam_map_options")
    for k, v in fields.items():
        if k not in dict(IbaFloamMapOptions._fields_):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def make_pairs(pairs):
    """[(src_edge_frame, src_surf_frame, map_edge_frame, map_surf_frame, T 4x4)] -> an array of iba_floam_pair"""
    arr = (IbaFloamPair * max(len(pairs), 1))()
    for a, (se, ss, me, ms, T) in zip(arr, pairs):
        a.src_edge_frame, a.src_surf_frame, a.map_edge_frame, a.map_surf_frame = int(se), int(ss), int(me), int(ms)
        a.T[:] = list(np.asarray(T, np.float64).reshape(16))
    return arr


def _n_points(handle, pairs):
    """source points per pair (edge cloud + surf cloud), or None when a frame is outside the handle (the library then refuses the call)"""
    out = []
    for p in pairs:
        a, b = handle.frame_num_points(int(p[0])), handle.frame_num_points(int(p[1]))
        if a < 0 or b < 0:
            return None
        out.append(a + b)
    return out


def step(handle, pairs, opt=None, nn=False, records=False, **fields):
    """iba_floam_map_step: pairs as for make_pairs -> moments [B, NMOM] (and, when asked, a list per pair of nn_idx [n, 5] uint32 and / or of
    records [n] RECORD_DTYPE, the pair's edge cloud first, then its surf cloud, each in original point order)"""
    L = _lib()
    o = map_options(**fields) if opt is None else opt
    B = len(pairs)
    arr = make_pairs(pairs)
    mom = np.zeros((max(B, 1), NMOM))
    counts = _n_points(handle, pairs) if (nn or records) else None
    n = int(sum(counts)) if counts else 0
    nn_buf = np.full((max(n, 1), 5), NONE, np.uint32) if nn and counts is not None else None
    rec_buf = np.zeros(max(n, 1), RECORD_DTYPE) if records and counts is not None else None
    handle._chk(L.iba_floam_map_step(handle.h, C.byref(arr), C.c_int32(B), C.byref(o), mom.ctypes.data_as(C.c_void_p),
                                     nn_buf.ctypes.data_as(C.c_void_p) if nn_buf is not None else None, rec_buf.ctypes.data_as(C.c_void_p) if rec_buf is not None else None))
    out = [mom[:B]]
    off = np.r_[0, np.cumsum(counts)] if counts is not None else None
    if nn:
        out.append([nn_buf[off[b]:off[b + 1]] for b in range(B)])
    if records:
        out.append([rec_buf[off[b]:off[b + 1]] for b in range(B)])
    return out[0] if len(out) == 1 else tuple(out)


def register(handle, pairs, opt=None, **fields):
    """iba_floam_map_register: pairs as for make_pairs -> list of dict(T [4, 4], initial_cost, final_cost, passes, iterations, evaluations, n_edge,
    n_surf, status) per pair"""
    L = _lib()
    o = map_options(**fields) if opt is None else opt
    B = len(pairs)
    arr = make_pairs(pairs)
    res = (IbaFloamMapResult * max(B, 1))()
    handle._chk(L.iba_floam_map_register(handle.h, C.byref(arr), C.c_int32(B), C.byref(o), C.byref(res)))
    return [dict(T=np.array(r.T[:]).reshape(4, 4), initial_cost=r.initial_cost, final_cost=r.final_cost, passes=r.passes, iterations=r.iterations,
                 evaluations=r.evaluations, n_edge=r.n_edge, n_surf=r.n_surf, status=r.status) for r in res[:B]]
