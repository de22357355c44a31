"""ctypes mirror of the map-point fusion (include/iba_mi355x.h, iba_fuse*; csrc/iba_fuse.hip): jobs and options, the batch call on the device or
through the host restatement, the result object with its accessors, and the host-only fold with its helpers over a FuseMap. Frames are
orb_match.frame(), the point table map_match.points(). Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last
from .orb_match import IbaOrbFrame

PICKED, SKIPPED, DEPTH, NOT_FINITE, BOUNDS, DISTANCE, ANGLE, NO_CANDIDATE, NO_MATCH = range(9)
N_STATUS = 9
LOCAL, LOOP = 0, 1
OP_NONE, OP_ADD, OP_REPLACED_BY_HELD, OP_REPLACES_HELD, OP_HELD_BAD, OP_RECORD, OP_STALE_BAD, OP_STALE_IN_KEYFRAME = range(8)


class IbaFuseJob(C.Structure):
    _fields_ = [("frame", C.c_int32), ("n_levels", C.c_int32), ("n_points", C.c_int32), ("th", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("Tcw12", C.c_void_p), ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("points", C.c_void_p), ("skip", C.c_void_p)]


class IbaFuseOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("th_low", C.c_int32), ("view_cos_limit", C.c_float), ("chi2_mono", C.c_float), ("check_reprojection", C.c_int32),
                ("keep_stages", C.c_int32)]


class IbaFuseCounts(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("status", C.c_int32 * N_STATUS), ("n_candidates", C.c_int32), ("n_picked", C.c_int32)]


class IbaFuseMap(C.Structure):
    _fields_ = [("K", C.c_int32), ("kp_off", C.c_void_p), ("holder", C.c_void_p), ("P", C.c_int32), ("bad", C.c_void_p), ("replaced_by", C.c_void_p), ("found", C.c_void_p),
                ("visible", C.c_void_p), ("descriptor_stale", C.c_void_p)]


def _lib():
    L = load_library()
    L.iba_fuse_last_error.restype = C.c_char_p
    L.iba_fuse_last_error.argtypes = []
    L.iba_default_fuse_options.argtypes = [C.c_void_p]
    L.iba_fuse.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_debug_fuse_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_fusion_free.argtypes = [C.c_void_p]
    L.iba_fusion_free.restype = None
    L.iba_fusion_n_jobs.argtypes = [C.c_void_p]
    L.iba_fusion_job.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_fusion_read.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
    L.iba_fusion_lists.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_fuse_apply.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_fuse_skip.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_fuse_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_debug_fuse_chunks.argtypes = [C.c_void_p]
    L.iba_debug_fuse_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_fuse_last_error")


def fuse_options(**fields):
    """iba_default_fuse_options with fields overridden"""
    L = _lib()
    return options_from(IbaFuseOptions, L.iba_default_fuse_options, L.iba_fuse_last_error, **fields)


def job(frame, Tcw, K, scale_factors, inv_level_sigma2, th, n_points, points=None, skip=None):
    """an IbaFuseJob over copies of the arrays (kept alive by the struct): Tcw [3, 4] or [4, 4] f32, K = (fx, fy, cx, cy), points = None (all
    n_points = P of the table in order) or [n_points] i32 (an entry < 0: no point), skip = None or [n_points] u8"""
    j = IbaFuseJob()
    j._keep = (np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12]).copy(), np.ascontiguousarray(scale_factors, np.float32).reshape(-1).copy(),
               np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1).copy(), None if points is None else np.ascontiguousarray(points, np.int32).reshape(-1).copy(),
               None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(-1).copy())
    T, sf, lv, pl, sk = j._keep
    assert len(lv) == len(sf) and (pl is None or len(pl) == n_points) and (sk is None or len(sk) == n_points)
    j.frame, j.n_levels, j.n_points, j.th = int(frame), len(sf), int(n_points), float(th)
    j.fx, j.fy, j.cx, j.cy = (float(v) for v in K)
    j.Tcw12, j.scale_factors, j.inv_level_sigma2 = T.ctypes.data, sf.ctypes.data, lv.ctypes.data
    j.points = pl.ctypes.data if pl is not None else None            # (an empty list is still a list)
    j.skip = sk.ctypes.data if sk is not None and len(sk) else None
    return j


class FuseMap:
    """iba_fuse_map over arrays of its own, which the fold changes in place: kp_off [K + 1] i32, holder [kp_off[K]] i32, bad [P] u8, replaced_by [P]
    i32, and found, visible [P] i32, descriptor_stale [P] u8 (or None)"""

    def __init__(self, kp_off, holder, P, bad=None, replaced_by=None, found=None, visible=None, descriptor_stale=True):
        self.kp_off = np.ascontiguousarray(kp_off, np.int32).copy()
        self.holder = np.ascontiguousarray(holder, np.int32).copy()
        self.P = int(P)
        self.bad = np.zeros(self.P, np.uint8) if bad is None else np.ascontiguousarray(bad, np.uint8).copy()
        self.replaced_by = np.full(self.P, -1, np.int32) if replaced_by is None else np.ascontiguousarray(replaced_by, np.int32).copy()
        self.found = None if found is None else np.ascontiguousarray(found, np.int32).copy()
        self.visible = None if visible is None else np.ascontiguousarray(visible, np.int32).copy()
        self.descriptor_stale = np.zeros(self.P, np.uint8) if descriptor_stale else None

    def struct(self):
        m = IbaFuseMap()
        m.K, m.P = len(self.kp_off) - 1, self.P
        m.kp_off, m.holder = self.kp_off.ctypes.data, self.holder.ctypes.data if len(self.holder) else None
        data = lambda a: a.ctypes.data if a is not None and len(a) else None
        m.bad, m.replaced_by, m.found, m.visible, m.descriptor_stale = data(self.bad), data(self.replaced_by), data(self.found), data(self.visible), data(self.descriptor_stale)
        return m

    def held(self, k):
        """the holder entries of keyframe k (a view)"""
        return self.holder[self.kp_off[k]:self.kp_off[k + 1]]


def skip(fmap, keyframe, points):
    """iba_fuse_skip -> [n] u8"""
    L = _lib()
    pl = np.ascontiguousarray(points, np.int32).reshape(-1)
    out = np.zeros(len(pl), np.uint8)
    m = fmap.struct()
    st = L.iba_fuse_skip(C.addressof(m), C.c_int32(keyframe), _p(pl) if len(pl) else None, C.c_int32(len(pl)), _p(out) if len(pl) else None)
    if st != 0:
        _raise(L, st)
    return out


def candidates(fmap, targets):
    """iba_fuse_candidates -> the list [n] i32"""
    L = _lib()
    tg = np.ascontiguousarray(targets, np.int32).reshape(-1)
    out, n = np.zeros(max(fmap.P, 1), np.int32), C.c_int32(0)
    m = fmap.struct()
    st = L.iba_fuse_candidates(C.addressof(m), _p(tg) if len(tg) else None, C.c_int32(len(tg)), _p(out), C.addressof(n))
    if st != 0:
        _raise(L, st)
    return out[:n.value].copy()


class Fusion(Result):
    """iba_fusion wrapper: the results of the jobs of one iba_fuse; close() it"""
    FREE, LAST_ERROR = "iba_fusion_free", "iba_fuse_last_error"

    def __len__(self):
        return int(self.lib.iba_fusion_n_jobs(self.p))

    @property
    def n_chunks(self):
        return int(self.lib.iba_debug_fuse_chunks(self.p))

    @property
    def stage_ms(self):
        """iba_debug_fuse_stage_ms: (frustum, grid + list count, scan + list write, pick) in ms; zeros unless IBA_FUSE_TIMING was set"""
        ms = np.zeros(4, np.float32)
        self._chk(self.lib.iba_debug_fuse_stage_ms(self.p, _p(ms)))
        return ms

    def counts(self, job):
        """-> dict: n_points, status [9] (by status code), n_candidates, n_picked"""
        c = IbaFuseCounts()
        self._chk(self.lib.iba_fusion_job(self.p, C.c_int32(job), C.addressof(c)))
        return {"n_points": c.n_points, "status": np.array(c.status[:], np.int32), "n_candidates": c.n_candidates, "n_picked": c.n_picked}

    def read(self, job):
        """-> dict per listed point: status u8, u, v f32, level i32, radius f32, match i32 (the keypoint or -1), dist i32"""
        n = self.counts(job)["n_points"]
        d = {"status": np.zeros(n, np.uint8), "u": np.zeros(n, np.float32), "v": np.zeros(n, np.float32), "level": np.zeros(n, np.int32), "radius": np.zeros(n, np.float32),
             "match": np.zeros(n, np.int32), "dist": np.zeros(n, np.int32)}
        self._chk(self.lib.iba_fusion_read(self.p, C.c_int32(job), *[_p(a) for a in d.values()]))
        return d

    def lists(self, job):
        """keep_stages -> (off [n_points + 1], index [n_candidates] i32, dist [n_candidates] u16) in M3's order"""
        c = self.counts(job)
        off, idx, d = np.zeros(c["n_points"] + 1, np.int32), np.zeros(c["n_candidates"], np.int32), np.zeros(c["n_candidates"], np.uint16)
        self._chk(self.lib.iba_fusion_lists(self.p, C.c_int32(job), _p(off), _p(idx), _p(d)))
        return off, idx, d

    def apply(self, job, keyframe, fmap, mode=LOCAL):
        """iba_fuse_apply: the fold of one job into fmap (changed in place) -> (op [n_points] i32, other [n_points] i32, n_fused)"""
        n = self.counts(job)["n_points"]
        op, other, nf = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int32(0)
        m = fmap.struct()
        self._chk(self.lib.iba_fuse_apply(self.p, C.c_int32(job), C.c_int32(keyframe), C.addressof(m), C.c_int32(mode), _p(op), _p(other), C.addressof(nf)))
        return op, other, nf.value


def _call(frames, table, jobs, opt, device, host, fields):
    L = _lib()
    o = fuse_options(**fields) if opt is None else opt
    fa = (IbaOrbFrame * max(len(frames), 1))()
    for i, f in enumerate(frames):
        C.memmove(C.addressof(fa[i]), C.addressof(f), C.sizeof(IbaOrbFrame))
    ja = (IbaFuseJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        C.memmove(C.addressof(ja[i]), C.addressof(j), C.sizeof(IbaFuseJob))
    p = C.c_void_p(None)
    head = [C.addressof(fa), C.c_int32(len(frames)), None if table is None else C.addressof(table), C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o)]
    st = L.iba_debug_fuse_host(*head, C.addressof(p)) if host else L.iba_fuse(*head, C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return Fusion(L, p)


def fuse(frames, table, jobs, opt=None, device=0, **fields):
    """iba_fuse: frames = a list of IbaOrbFrame (orb_match.frame()), table = map_match.points(), jobs = a list of IbaFuseJob (job()) -> Fusion.
    opt = an IbaFuseOptions, or fields of one over the defaults."""
    return _call(frames, table, jobs, opt, device, False, fields)


def fuse_host(frames, table, jobs, opt=None, **fields):
    """iba_debug_fuse_host: the same call through the host restatement of the rules, no device"""
    return _call(frames, table, jobs, opt, 0, True, fields)
