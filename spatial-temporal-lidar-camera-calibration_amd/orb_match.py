"""ctypes mirror of the windowed ORB matching (include/iba_mi355x.h, iba_orb_match*; csrc/iba_orb_match.hip): frames, jobs and options, the batch
call, the result object with its stage accessors, and the two host-only query builders. Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last

INIT, CLAIM = 0, 1
N_CELLS, HISTO = 64 * 48, 30


class IbaOrbFrame(C.Structure):
    _fields_ = [("xy", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int32),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class IbaOrbMatchJob(C.Structure):
    _fields_ = [("query_frame", C.c_int32), ("train_frame", C.c_int32), ("rule", C.c_int32), ("n_queries", C.c_int32), ("centre_xy", C.c_void_p),
                ("radius", C.c_void_p), ("level_range", C.c_void_p), ("query_index", C.c_void_p), ("valid", C.c_void_p)]


class IbaOrbMatchOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("th_low", C.c_int32), ("th_high", C.c_int32), ("nn_ratio", C.c_float), ("check_orientation", C.c_int32),
                ("keep_stages", C.c_int32)]


class IbaOrbMatchCounts(C.Structure):
    _fields_ = [("n_queries", C.c_int32), ("n_matches", C.c_int32), ("n_candidates", C.c_int32), ("n_displaced", C.c_int32), ("n_rot_removed", C.c_int32),
                ("hist", C.c_int32 * HISTO), ("ind", C.c_int32 * 3)]


def _lib():
    L = load_library()
    L.iba_orb_match_last_error.restype = C.c_char_p
    L.iba_orb_match_last_error.argtypes = []
    L.iba_default_orb_match_options.argtypes = [C.POINTER(IbaOrbMatchOptions)]
    L.iba_orb_match.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_orb_matches_free.argtypes = [C.c_void_p]
    L.iba_orb_matches_free.restype = None
    L.iba_orb_matches_n_jobs.argtypes = [C.c_void_p]
    L.iba_orb_matches_job.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_orb_matches_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_orb_matches_grid.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_orb_matches_lists.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_orb_match_init_queries.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    L.iba_orb_match_motion_queries.argtypes = [C.c_void_p] * 5 + [C.c_float] * 4 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_float] + [C.c_void_p] * 5
    L.iba_debug_orb_match_stub.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.iba_debug_orb_match_chunks.argtypes = [C.c_void_p]
    L.iba_debug_orb_match_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.iba_debug_orb_match_plan.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_orb_match_last_error")


def match_options(**fields):
    """iba_default_orb_match_options with fields overridden"""
    L = _lib()
    return options_from(IbaOrbMatchOptions, L.iba_default_orb_match_options, L.iba_orb_match_last_error, **fields)


def frame(xy, octave, angle, desc, bounds):
    """an IbaOrbFrame over copies of the arrays (kept alive by the struct): xy [n, 2] f32, octave [n] i32, angle [n] f32 degrees, desc [n, 32] u8,
    bounds = (min_x, max_x, min_y, max_y)"""
    f = IbaOrbFrame()
    f._keep = (np.ascontiguousarray(xy, np.float32).reshape(-1, 2), np.ascontiguousarray(octave, np.int32).reshape(-1),
               np.ascontiguousarray(angle, np.float32).reshape(-1), np.ascontiguousarray(desc, np.uint8).reshape(-1, 32))
    n = len(f._keep[1])
    assert len(f._keep[0]) == n and len(f._keep[2]) == n and len(f._keep[3]) == n
    f.xy, f.octave, f.angle, f.desc = (a.ctypes.data if n else None for a in f._keep)
    f.n = n
    f.min_x, f.max_x, f.min_y, f.max_y = (float(v) for v in bounds)
    return f


def job(query_frame, train_frame, rule, centre_xy, radius, level_range, query_index, valid=None):
    """an IbaOrbMatchJob over copies of the per-query arrays (kept alive by the struct)"""
    j = IbaOrbMatchJob()
    j._keep = (np.ascontiguousarray(centre_xy, np.float32).reshape(-1, 2), np.ascontiguousarray(radius, np.float32).reshape(-1),
               np.ascontiguousarray(level_range, np.int32).reshape(-1, 2), np.ascontiguousarray(query_index, np.int32).reshape(-1),
               None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(-1))
    n = len(j._keep[1])
    assert all(a is None or len(a) == n for a in j._keep)
    j.query_frame, j.train_frame, j.rule, j.n_queries = int(query_frame), int(train_frame), int(rule), n
    j.centre_xy, j.radius, j.level_range, j.query_index = (a.ctypes.data if n else None for a in j._keep[:4])
    j.valid = j._keep[4].ctypes.data if (j._keep[4] is not None and n) else None
    return j


def _query_outputs(n):
    return {"centre_xy": np.zeros((n, 2), np.float32), "radius": np.zeros(n, np.float32), "level_range": np.zeros((n, 2), np.int32),
            "query_index": np.zeros(n, np.int32), "valid": np.zeros(n, np.uint8)}


_ORDER = ("centre_xy", "radius", "level_range", "query_index", "valid")


def init_queries(frame1, prev_matched_xy, window_size):
    """iba_orb_match_init_queries (host only) -> dict of the per-query arrays, the keyword arguments of job()"""
    L = _lib()
    prev = None if prev_matched_xy is None else np.ascontiguousarray(prev_matched_xy, np.float32).reshape(-1, 2)
    out = _query_outputs(frame1.n if frame1 is not None else 0)
    st = L.iba_orb_match_init_queries(None if frame1 is None else C.addressof(frame1), _p(prev), C.c_int32(window_size), *[_p(out[k]) for k in _ORDER])
    if st != 0:
        _raise(L, st)
    return out


def motion_queries(last_frame, has_point, outlier, world_xyz, Tcw, fx, fy, cx, cy, bounds, scale_factors, th):
    """iba_orb_match_motion_queries (host only): Tcw = the current frame's pose (3 x 4 or 4 x 4, row-major), bounds = the current frame's
    (min_x, max_x, min_y, max_y) -> dict of the per-query arrays"""
    L = _lib()
    hp, ol = np.ascontiguousarray(has_point, np.uint8).reshape(-1), np.ascontiguousarray(outlier, np.uint8).reshape(-1)
    X = np.ascontiguousarray(world_xyz, np.float32).reshape(-1, 3)
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
    b, sf = np.ascontiguousarray(bounds, np.float32).reshape(4), np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    out = _query_outputs(last_frame.n)
    assert len(hp) == last_frame.n and len(ol) == last_frame.n and len(X) == last_frame.n
    st = L.iba_orb_match_motion_queries(C.addressof(last_frame), _p(hp), _p(ol), _p(X), _p(T), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), _p(b), _p(sf),
                                        C.c_int32(len(sf)), C.c_float(th), *[_p(out[k]) for k in _ORDER])
    if st != 0:
        _raise(L, st)
    return out


def plan_chunks(candidates, budget):
    """iba_debug_orb_match_plan (host only): the cut of the jobs under a byte budget -> ascending job indices, first 0, last len(candidates)"""
    L = _lib()
    c = np.ascontiguousarray(candidates, np.int64).reshape(-1)
    cut, n = np.zeros(len(c) + 1, np.int32), C.c_int32(0)
    st = L.iba_debug_orb_match_plan(_p(c), C.c_int32(len(c)), C.c_uint64(budget), _p(cut), C.addressof(n))
    if st != 0:
        _raise(L, st)
    return cut[:n.value].copy()


class OrbMatches(Result):
    """iba_orb_matches wrapper: the results of the jobs of one iba_orb_match; close() it"""
    FREE, LAST_ERROR = "iba_orb_matches_free", "iba_orb_match_last_error"

    def __init__(self, lib, p, frame_n):
        super().__init__(lib, p)
        self.frame_n = frame_n

    @classmethod
    def stub(cls, n_jobs, n_frames, keep_stages=0):
        """iba_debug_orb_match_stub (host only): empty jobs over empty frames"""
        L = _lib()
        p = C.c_void_p(None)
        st = L.iba_debug_orb_match_stub(C.c_int32(n_jobs), C.c_int32(n_frames), C.c_int32(keep_stages), C.addressof(p))
        if st != 0:
            _raise(L, st)
        return cls(L, p, [0] * n_frames)

    def __len__(self):
        return int(self.lib.iba_orb_matches_n_jobs(self.p))

    @property
    def n_chunks(self):
        return int(self.lib.iba_debug_orb_match_chunks(self.p))

    @property
    def stage_ms(self):
        """iba_debug_orb_match_stage_ms: (grid, list count, scan + list write, resolve) in ms; zeros unless IBA_ORB_MATCH_TIMING was set"""
        ms = np.zeros(4, np.float32)
        self._chk(self.lib.iba_debug_orb_match_stage_ms(self.p, _p(ms)))
        return ms

    def counts(self, job):
        """-> dict: n_queries, n_matches, n_candidates, n_displaced, n_rot_removed, hist [30], ind [3]"""
        c = IbaOrbMatchCounts()
        self._chk(self.lib.iba_orb_matches_job(self.p, C.c_int32(job), C.addressof(c)))
        return {"n_queries": c.n_queries, "n_matches": c.n_matches, "n_candidates": c.n_candidates, "n_displaced": c.n_displaced, "n_rot_removed": c.n_rot_removed,
                "hist": np.array(c.hist[:], np.int32), "ind": np.array(c.ind[:], np.int32)}

    def read(self, job):
        """-> (match [n_queries] i32: the train index or -1, dist [n_queries] i32: the accepted distance or -1)"""
        n = self.counts(job)["n_queries"]
        match, dist = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._chk(self.lib.iba_orb_matches_read(self.p, C.c_int32(job), _p(match), _p(dist)))
        return match, dist

    def grid(self, frame):
        """keep_stages -> (cell_off [3073] with cell = px * 48 + py, list [cell_off[3072]])"""
        n = self.frame_n[frame] if 0 <= frame < len(self.frame_n) else 0
        off, lst, k = np.zeros(N_CELLS + 1, np.int32), np.zeros(n, np.int32), C.c_int32(0)
        self._chk(self.lib.iba_orb_matches_grid(self.p, C.c_int32(frame), _p(off), _p(lst), C.addressof(k)))
        return off, lst[:k.value].copy()

    def lists(self, job):
        """keep_stages -> (off [n_queries + 1], index [n_candidates] i32, dist [n_candidates] u16) in M3's order"""
        c = self.counts(job)
        off, idx, d = np.zeros(c["n_queries"] + 1, np.int32), np.zeros(c["n_candidates"], np.int32), np.zeros(c["n_candidates"], np.uint16)
        self._chk(self.lib.iba_orb_matches_lists(self.p, C.c_int32(job), _p(off), _p(idx), _p(d)))
        return off, idx, d


def match(frames, jobs, opt=None, device=0, **fields):
    """iba_orb_match: frames = a list of IbaOrbFrame (frame()), jobs = a list of IbaOrbMatchJob (job()) -> OrbMatches. opt = an IbaOrbMatchOptions, or
    fields of one over the defaults."""
    L = _lib()
    o = match_options(**fields) if opt is None else opt
    fa = (IbaOrbFrame * max(len(frames), 1))()
    for i, f in enumerate(frames):
        C.memmove(C.addressof(fa[i]), C.addressof(f), C.sizeof(IbaOrbFrame))
    ja = (IbaOrbMatchJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        C.memmove(C.addressof(ja[i]), C.addressof(j), C.sizeof(IbaOrbMatchJob))
    p = C.c_void_p(None)
    st = L.iba_orb_match(C.addressof(fa), C.c_int32(len(frames)), C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o), C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return OrbMatches(L, p, [int(f.n) for f in frames])
