"""ctypes mirror of the local-map point matching (include/iba_mi355x.h, iba_map_match*; csrc/iba_map_match.hip): the point table, jobs and options,
the batch call on the device or through the host restatement, the result object with its accessors, and the host-only edge helper. Frames are
orb_match.frame(). Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last
from .orb_match import IbaOrbFrame

IN_VIEW, SKIPPED, DEPTH, NOT_FINITE, BOUNDS, DISTANCE, ANGLE = range(7)
N_STATUS, MAX_LEVELS = 7, 64


class IbaMapPoints(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int32)]


class IbaMapMatchJob(C.Structure):
    _fields_ = [("frame", C.c_int32), ("n_levels", C.c_int32), ("n_points", C.c_int32), ("th", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("Tcw12", C.c_void_p), ("scale_factors", C.c_void_p), ("points", C.c_void_p), ("skip", C.c_void_p), ("occupied", C.c_void_p)]


class IbaMapMatchOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("th_high", C.c_int32), ("nn_ratio", C.c_float), ("view_cos_limit", C.c_float), ("keep_stages", C.c_int32)]


class IbaMapMatchCounts(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("status", C.c_int32 * N_STATUS), ("n_candidates", C.c_int32), ("n_matches", C.c_int32)]


def _lib():
    L = load_library()
    L.iba_map_match_last_error.restype = C.c_char_p
    L.iba_map_match_last_error.argtypes = []
    L.iba_default_map_match_options.argtypes = [C.c_void_p]
    L.iba_map_match.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_debug_map_match_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_map_matches_free.argtypes = [C.c_void_p]
    L.iba_map_matches_free.restype = None
    L.iba_map_matches_n_jobs.argtypes = [C.c_void_p]
    L.iba_map_matches_job.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_map_matches_read.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
    L.iba_map_matches_keypoints.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_map_matches_lists.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_map_match_pose_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    L.iba_debug_map_match_chunks.argtypes = [C.c_void_p]
    L.iba_debug_map_match_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_map_match_last_error")


def match_options(**fields):
    """iba_default_map_match_options with fields overridden"""
    L = _lib()
    return options_from(IbaMapMatchOptions, L.iba_default_map_match_options, L.iba_map_match_last_error, **fields)


def points(xyz, normal, min_dist, max_dist, desc):
    """an IbaMapPoints over copies of the arrays (kept alive by the struct): xyz, normal [P, 3] f32, min_dist, max_dist [P] f32, desc [P, 32] u8"""
    t = IbaMapPoints()
    t._keep = (np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).copy(), np.ascontiguousarray(normal, np.float32).reshape(-1, 3).copy(),
               np.ascontiguousarray(min_dist, np.float32).reshape(-1).copy(), np.ascontiguousarray(max_dist, np.float32).reshape(-1).copy(),
               np.ascontiguousarray(desc, np.uint8).reshape(-1, 32).copy())
    n = len(t._keep[2])
    assert all(len(a) == n for a in t._keep)
    t.xyz, t.normal, t.min_dist, t.max_dist, t.desc = (a.ctypes.data if n else None for a in t._keep)
    t.n = n
    return t


def job(frame, Tcw, K, scale_factors, th, n_points, points=None, skip=None, occupied=None):
    """an IbaMapMatchJob over copies of the arrays (kept alive by the struct): Tcw [3, 4] or [4, 4] f32, K = (fx, fy, cx, cy), points = None (all
    n_points = P of the table in order) or [n_points] i32, skip = None or [n_points] u8, occupied = None or one byte per keypoint of the frame"""
    j = IbaMapMatchJob()
    j._keep = (np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12]).copy(), np.ascontiguousarray(scale_factors, np.float32).reshape(-1).copy(),
               None if points is None else np.ascontiguousarray(points, np.int32).reshape(-1).copy(), None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(-1).copy(),
               None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(-1).copy())
    T, sf, pl, sk, oc = j._keep
    assert (pl is None or len(pl) == n_points) and (sk is None or len(sk) == n_points)
    j.frame, j.n_levels, j.n_points, j.th = int(frame), len(sf), int(n_points), float(th)
    j.fx, j.fy, j.cx, j.cy = (float(v) for v in K)
    j.Tcw12, j.scale_factors = T.ctypes.data, sf.ctypes.data
    j.points = pl.ctypes.data if pl is not None else None            # (an empty list is still a list)
    j.skip = sk.ctypes.data if sk is not None and len(sk) else None
    j.occupied = oc.ctypes.data if oc is not None and len(oc) else None
    return j


class MapMatches(Result):
    """iba_map_matches wrapper: the results of the jobs of one iba_map_match; close() it"""
    FREE, LAST_ERROR = "iba_map_matches_free", "iba_map_match_last_error"

    def __init__(self, lib, p, frame_n):
        super().__init__(lib, p)
        self.frame_n = frame_n            # per job: the keypoints of its frame

    def __len__(self):
        return int(self.lib.iba_map_matches_n_jobs(self.p))

    @property
    def n_chunks(self):
        return int(self.lib.iba_debug_map_match_chunks(self.p))

    @property
    def stage_ms(self):
        """iba_debug_map_match_stage_ms: (frustum, grid + list count, scan + list write, resolve) in ms; zeros unless IBA_MAP_MATCH_TIMING was set"""
        ms = np.zeros(4, np.float32)
        self._chk(self.lib.iba_debug_map_match_stage_ms(self.p, _p(ms)))
        return ms

    def counts(self, job):
        """-> dict: n_points, status [7] (by status code), n_candidates, n_matches"""
        c = IbaMapMatchCounts()
        self._chk(self.lib.iba_map_matches_job(self.p, C.c_int32(job), C.addressof(c)))
        return {"n_points": c.n_points, "status": np.array(c.status[:], np.int32), "n_candidates": c.n_candidates, "n_matches": c.n_matches}

    def read(self, job):
        """-> dict per listed point: status u8, u, v, view_cos f32, level i32, radius f32, match i32 (the keypoint or -1), dist i32"""
        n = self.counts(job)["n_points"]
        d = {"status": np.zeros(n, np.uint8), "u": np.zeros(n, np.float32), "v": np.zeros(n, np.float32), "view_cos": np.zeros(n, np.float32), "level": np.zeros(n, np.int32),
             "radius": np.zeros(n, np.float32), "match": np.zeros(n, np.int32), "dist": np.zeros(n, np.int32)}
        self._chk(self.lib.iba_map_matches_read(self.p, C.c_int32(job), *[_p(a) for a in d.values()]))
        return d

    def keypoints(self, job):
        """-> point_of [n of the job's frame] i32: the position in the job's list that claimed the keypoint, or -1"""
        n = self.frame_n[job] if 0 <= job < len(self.frame_n) else 0
        po = np.zeros(n, np.int32)
        self._chk(self.lib.iba_map_matches_keypoints(self.p, C.c_int32(job), _p(po)))
        return po

    def lists(self, job):
        """keep_stages -> (off [n_points + 1], index [n_candidates] i32, dist [n_candidates] u16) in M3's order"""
        c = self.counts(job)
        off, idx, d = np.zeros(c["n_points"] + 1, np.int32), np.zeros(c["n_candidates"], np.int32), np.zeros(c["n_candidates"], np.uint16)
        self._chk(self.lib.iba_map_matches_lists(self.p, C.c_int32(job), _p(off), _p(idx), _p(d)))
        return off, idx, d


def _call(frames, table, jobs, opt, device, host, fields):
    L = _lib()
    o = match_options(**fields) if opt is None else opt
    fa = (IbaOrbFrame * max(len(frames), 1))()
    for i, f in enumerate(frames):
        C.memmove(C.addressof(fa[i]), C.addressof(f), C.sizeof(IbaOrbFrame))
    ja = (IbaMapMatchJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        C.memmove(C.addressof(ja[i]), C.addressof(j), C.sizeof(IbaMapMatchJob))
    p = C.c_void_p(None)
    head = [C.addressof(fa), C.c_int32(len(frames)), None if table is None else C.addressof(table), C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o)]
    st = L.iba_debug_map_match_host(*head, C.addressof(p)) if host else L.iba_map_match(*head, C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return MapMatches(L, p, [int(frames[j.frame].n) for j in jobs])


def match(frames, table, jobs, opt=None, device=0, **fields):
    """iba_map_match: frames = a list of IbaOrbFrame (orb_match.frame()), table = points(), jobs = a list of IbaMapMatchJob (job()) -> MapMatches.
    opt = an IbaMapMatchOptions, or fields of one over the defaults."""
    return _call(frames, table, jobs, opt, device, False, fields)


def match_host(frames, table, jobs, opt=None, **fields):
    """iba_debug_map_match_host: the same call through the host restatement of the rules, no device"""
    return _call(frames, table, jobs, opt, 0, True, fields)


def pose_edges(prior_point, point_of, points, n_points, table_xyz, xy, octave, inv_level_sigma2):
    """iba_map_match_pose_edges (host only, rule L6) -> (xyz [n, 3] f32, obs [n, 2] f32, inv_sigma2 [n] f32, keypoint_index [n] i32): the arrays of
    pose.job(). prior_point, point_of: [n_kp] i32 or None; points: the job's list or None"""
    L = _lib()
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).reshape(-1)
    pp, po, pl = i32(prior_point), i32(point_of), i32(points)
    tx = np.ascontiguousarray(table_xyz, np.float32).reshape(-1, 3)
    kxy, oc = np.ascontiguousarray(xy, np.float32).reshape(-1, 2), np.ascontiguousarray(octave, np.int32).reshape(-1)
    lv = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
    nk = len(kxy)
    assert len(oc) == nk and (pp is None or len(pp) == nk) and (po is None or len(po) == nk)
    xyz, obs, w, idx, n = np.zeros((nk, 3), np.float32), np.zeros((nk, 2), np.float32), np.zeros(nk, np.float32), np.zeros(nk, np.int32), C.c_int32(0)
    st = L.iba_map_match_pose_edges(_p(pp), _p(po), _p(pl), C.c_int32(n_points), _p(tx) if len(tx) else None, C.c_int32(len(tx)), _p(kxy) if nk else None, _p(oc) if nk else None,
                                    C.c_int32(nk), _p(lv) if len(lv) else None, C.c_int32(len(lv)), _p(xyz) if nk else None, _p(obs) if nk else None, _p(w) if nk else None,
                                    _p(idx) if nk else None, C.addressof(n))
    if st != 0:
        _raise(L, st)
    return xyz[:n.value], obs[:n.value], w[:n.value], idx[:n.value]
