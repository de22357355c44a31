"""ctypes mirror of the F-LOAM feature extraction (include/iba_mi355x.h, iba_floam_*; csrc/iba_floam_host.hpp): the edge cloud and the surf cloud
of a batch of resident scans. Plumbing only."""
import ctypes as C

import numpy as np

from . import IbaError, load_library
from .abi import FLOAM_MAX_RING_POINTS, IbaFloamOptions   # noqa: F401

MAX_RING_POINTS = FLOAM_MAX_RING_POINTS


def _lib():
    L = load_library()
    L.iba_default_floam_options.argtypes = [C.c_void_p]
    L.iba_floam_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.iba_floam_num.argtypes = [C.c_void_p]; L.iba_floam_num.restype = C.c_int32
    for f, rt in ((L.iba_floam_n_edge, C.c_int64), (L.iba_floam_n_surf, C.c_int64), (L.iba_floam_edge_xyz, C.POINTER(C.c_float)), (L.iba_floam_surf_xyz, C.POINTER(C.c_float)),
                  (L.iba_floam_edge_index, C.POINTER(C.c_int32)), (L.iba_floam_surf_index, C.POINTER(C.c_int32))):
        f.argtypes = [C.c_void_p, C.c_int32]; f.restype = rt
    L.iba_floam_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
    L.iba_floam_free.argtypes = [C.c_void_p]; L.iba_floam_free.restype = None
    return L


def floam_options(**fields):
    """iba_default_floam_options (the reference's constants) with fields overridden"""
    o = IbaFloamOptions()
    st = _lib().iba_default_floam_options(C.byref(o))
    if st != 0:
        raise IbaError(st, "iba_default_floam_options")
    for k, v in fields.items():
        if k not in dict(IbaFloamOptions._fields_):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def extract(handle, frames, opt=None, **fields):
    """iba_floam_extract on an IbaHandle: local frames [n] -> list of dict(edge_xyz [E, 3] float32, edge_index [E] int32, surf_xyz [S, 3] float32,
    surf_index [S] int32, n_nonfinite, n_out_of_range, n_no_ring, ring_points [num_lines] int32) per scan"""
    L = _lib()
    o = floam_options(**fields) if opt is None else opt
    fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
    res = C.c_void_p(None)
    handle._chk(L.iba_floam_extract(handle.h, fr.ctypes.data_as(C.c_void_p) if len(fr) else None, C.c_int32(len(fr)), C.byref(o), C.byref(res)))
    try:
        out = []
        for s in range(L.iba_floam_num(res)):
            ne, ns = int(L.iba_floam_n_edge(res, s)), int(L.iba_floam_n_surf(res, s))
            d = dict(edge_xyz=np.ctypeslib.as_array(L.iba_floam_edge_xyz(res, s), shape=(ne, 3)).copy() if ne else np.zeros((0, 3), np.float32),
                     edge_index=np.ctypeslib.as_array(L.iba_floam_edge_index(res, s), shape=(ne,)).copy() if ne else np.zeros(0, np.int32),
                     surf_xyz=np.ctypeslib.as_array(L.iba_floam_surf_xyz(res, s), shape=(ns, 3)).copy() if ns else np.zeros((0, 3), np.float32),
                     surf_index=np.ctypeslib.as_array(L.iba_floam_surf_index(res, s), shape=(ns,)).copy() if ns else np.zeros(0, np.int32))
            a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            rings = np.zeros(int(o.num_lines), np.int32)
            handle._chk(L.iba_floam_stats(res, s, C.byref(a), C.byref(b), C.byref(c), rings.ctypes.data_as(C.c_void_p)))
            d.update(n_nonfinite=a.value, n_out_of_range=b.value, n_no_ring=c.value, ring_points=rings)
            out.append(d)
    finally:
        L.iba_floam_free(res)
    return out
