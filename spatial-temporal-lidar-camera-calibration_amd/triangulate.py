"""ctypes mirror of the new-map-point creation (include/iba_mi355x.h, iba_triangulate*; csrc/iba_triangulate.hip): keyframes, jobs and options, the
batch call on the device or through the host restatement, the result object with its accessors, and the host-only median depth. Frames are
orb_match.frame(). Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last
from .orb_match import IbaOrbFrame

(CREATED, HAS_POINT, NO_NODE, PAIR_SKIPPED, NO_MATCH, PARALLAX, DEGENERATE, DEPTH1, DEPTH2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, SUPERSEDED) = range(14)
N_STATUS, MAX_LEVELS, BYTES_PER_SLOT = 14, 64, 120


class IbaTriangulateKeyframe(C.Structure):
    _fields_ = [("frame", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("median_depth", C.c_float), ("Tcw12", C.c_void_p),
                ("node", C.c_void_p), ("has_point", C.c_void_p)]


class IbaTriangulateJob(C.Structure):
    _fields_ = [("current", C.c_int32), ("n_neighbours", C.c_int32), ("n_levels", C.c_int32), ("scale_factor", C.c_float), ("neighbours", C.c_void_p), ("scale_factors", C.c_void_p),
                ("level_sigma2", C.c_void_p)]


class IbaTriangulateOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("th_low", C.c_int32), ("min_baseline_ratio", C.c_float), ("max_cos_parallax", C.c_float), ("epipole_gate", C.c_float),
                ("chi2_line", C.c_float), ("chi2_mono", C.c_float), ("keep_stages", C.c_int32)]


class IbaTriangulateCounts(C.Structure):
    _fields_ = [("n_keypoints", C.c_int32), ("n_neighbours", C.c_int32), ("status", C.c_int32 * N_STATUS), ("n_created", C.c_int32)]


def _lib():
    L = load_library()
    L.iba_triangulate_last_error.restype = C.c_char_p
    L.iba_triangulate_last_error.argtypes = []
    L.iba_default_triangulate_options.argtypes = [C.c_void_p]
    L.iba_triangulate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_debug_triangulate_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_triangulation_free.argtypes = [C.c_void_p]
    L.iba_triangulation_free.restype = None
    L.iba_triangulation_n_jobs.argtypes = [C.c_void_p]
    L.iba_triangulation_job.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_triangulation_read.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    L.iba_triangulation_points.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
    L.iba_triangulation_segments.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_triangulate_median_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.iba_debug_triangulate_chunks.argtypes = [C.c_void_p]
    L.iba_debug_triangulate_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_triangulate_last_error")


def triangulate_options(**fields):
    """iba_default_triangulate_options with fields overridden"""
    L = _lib()
    return options_from(IbaTriangulateOptions, L.iba_default_triangulate_options, L.iba_triangulate_last_error, **fields)


def keyframe(frame, Tcw, K, node, has_point=None, median_depth=1.0):
    """an IbaTriangulateKeyframe over copies of the arrays (kept alive by the struct): Tcw [3, 4] or [4, 4] f32, K = (fx, fy, cx, cy), node [n] i32,
    has_point = None or [n] u8"""
    k = IbaTriangulateKeyframe()
    k._keep = (np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12]).copy(), np.ascontiguousarray(node, np.int32).reshape(-1).copy(),
               None if has_point is None else np.ascontiguousarray(has_point, np.uint8).reshape(-1).copy())
    T, nd, hp = k._keep
    assert hp is None or len(hp) == len(nd)
    k.frame, k.median_depth = int(frame), float(median_depth)
    k.fx, k.fy, k.cx, k.cy = (float(v) for v in K)
    k.Tcw12 = T.ctypes.data
    k.node = nd.ctypes.data if len(nd) else None
    k.has_point = hp.ctypes.data if hp is not None and len(hp) else None
    return k


def job(current, neighbours, scale_factors, level_sigma2, scale_factor):
    """an IbaTriangulateJob over copies of the arrays (kept alive by the struct): neighbours [n_neighbours] i32 in covisibility order"""
    j = IbaTriangulateJob()
    j._keep = (np.ascontiguousarray(neighbours, np.int32).reshape(-1).copy(), np.ascontiguousarray(scale_factors, np.float32).reshape(-1).copy(),
               np.ascontiguousarray(level_sigma2, np.float32).reshape(-1).copy())
    nb, sf, s2 = j._keep
    assert len(sf) == len(s2)
    j.current, j.n_neighbours, j.n_levels, j.scale_factor = int(current), len(nb), len(sf), float(scale_factor)
    j.neighbours = nb.ctypes.data if len(nb) else None
    j.scale_factors, j.level_sigma2 = sf.ctypes.data, s2.ctypes.data
    return j


class Triangulation(Result):
    """iba_triangulation wrapper: the results of the jobs of one iba_triangulate; close() it"""
    FREE, LAST_ERROR = "iba_triangulation_free", "iba_triangulate_last_error"

    def __len__(self):
        return int(self.lib.iba_triangulation_n_jobs(self.p))

    @property
    def n_chunks(self):
        return int(self.lib.iba_debug_triangulate_chunks(self.p))

    @property
    def stage_ms(self):
        """iba_debug_triangulate_stage_ms: (prologue + segments, pick, compaction + triangulation, resolve + counts + scan + gather) in ms; zeros
        unless IBA_TRIANGULATE_TIMING was set"""
        ms = np.zeros(4, np.float32)
        self._chk(self.lib.iba_debug_triangulate_stage_ms(self.p, _p(ms)))
        return ms

    def counts(self, job):
        """-> dict: n_keypoints, n_neighbours, status [14] (by status code), n_created, and per neighbour n_matches, n_created_of"""
        c = IbaTriangulateCounts()
        self._chk(self.lib.iba_triangulation_job(self.p, C.c_int32(job), C.addressof(c), None, None))
        nm, nc = np.zeros(c.n_neighbours, np.int32), np.zeros(c.n_neighbours, np.int32)
        self._chk(self.lib.iba_triangulation_job(self.p, C.c_int32(job), C.addressof(c), _p(nm), _p(nc)))
        return {"n_keypoints": c.n_keypoints, "n_neighbours": c.n_neighbours, "status": np.array(c.status[:], np.int32), "n_created": c.n_created, "n_matches": nm, "n_created_of": nc}

    def read(self, job):
        """-> dict per slot [n_neighbours, n_keypoints]: status u8, match i32 (idx2 or -1), dist i32, xyz [.., 3] f32"""
        c = self.counts(job)
        shape = (c["n_neighbours"], c["n_keypoints"])
        d = {"status": np.zeros(shape, np.uint8), "match": np.zeros(shape, np.int32), "dist": np.zeros(shape, np.int32), "xyz": np.zeros(shape + (3,), np.float32)}
        self._chk(self.lib.iba_triangulation_read(self.p, C.c_int32(job), *[_p(a) for a in d.values()]))
        return d

    def points(self, job):
        """-> dict of the created points in creation order: idx1, neighbour, idx2 i32, xyz, normal [n, 3] f32, min_dist, max_dist f32, desc [n, 32] u8"""
        n = self.counts(job)["n_created"]
        d = {"idx1": np.zeros(n, np.int32), "neighbour": np.zeros(n, np.int32), "idx2": np.zeros(n, np.int32), "xyz": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32),
             "min_dist": np.zeros(n, np.float32), "max_dist": np.zeros(n, np.float32), "desc": np.zeros((n, 32), np.uint8)}
        self._chk(self.lib.iba_triangulation_points(self.p, C.c_int32(job), *[_p(a) for a in d.values()]))
        return d

    def segments(self, job):
        """keep_stages -> seg_len [n_neighbours, n_keypoints] i32"""
        c = self.counts(job)
        s = np.zeros((c["n_neighbours"], c["n_keypoints"]), np.int32)
        self._chk(self.lib.iba_triangulation_segments(self.p, C.c_int32(job), _p(s)))
        return s


def _array(Struct, items):
    a = (Struct * max(len(items), 1))()
    for i, x in enumerate(items):
        C.memmove(C.addressof(a[i]), C.addressof(x), C.sizeof(Struct))
    return a


def _call(frames, keyframes, jobs, opt, device, host, fields):
    L = _lib()
    o = triangulate_options(**fields) if opt is None else opt
    fa, ka, ja = _array(IbaOrbFrame, frames), _array(IbaTriangulateKeyframe, keyframes), _array(IbaTriangulateJob, jobs)
    p = C.c_void_p(None)
    head = [C.addressof(fa), C.c_int32(len(frames)), C.addressof(ka), C.c_int32(len(keyframes)), C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o)]
    st = L.iba_debug_triangulate_host(*head, C.addressof(p)) if host else L.iba_triangulate(*head, C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return Triangulation(L, p)


def triangulate(frames, keyframes, jobs, opt=None, device=0, **fields):
    """iba_triangulate: frames = a list of IbaOrbFrame (orb_match.frame()), keyframes = a list of keyframe(), jobs = a list of job() -> Triangulation.
    opt = an IbaTriangulateOptions, or fields of one over the defaults."""
    return _call(frames, keyframes, jobs, opt, device, False, fields)


def triangulate_host(frames, keyframes, jobs, opt=None, **fields):
    """iba_debug_triangulate_host: the same call through the host restatement of the rules, no device"""
    return _call(frames, keyframes, jobs, opt, 0, True, fields)


def median_depth(Tcw, xyz, q=2):
    """iba_triangulate_median_depth (host only): KeyFrame::ComputeSceneMedianDepth(q)"""
    L = _lib()
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
    X = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = C.c_float(0)
    st = L.iba_triangulate_median_depth(_p(T), _p(X) if len(X) else None, C.c_int32(len(X)), C.c_int32(q), C.addressof(out))
    if st != 0:
        _raise(L, st)
    return np.float32(out.value)
