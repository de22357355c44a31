"""ctypes mirror of the map-point refresh (include/iba_mi355x.h, iba_refresh*; csrc/iba_refresh.hip): keyframes and options, the batch call on the
device or through the host restatement, the result object with its accessors, and the two host-only helpers. Frames are orb_match.frame(), the
point table map_match.points(), the map of iba_refresh_observations a fuse.FuseMap. Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last
from .orb_match import IbaOrbFrame

REFRESHED, BAD, EMPTY = range(3)
DESC_NONE, DESC_PICKED, DESC_KEPT = range(3)
GEO_NONE, GEO_UPDATED, GEO_NO_REF, GEO_DEGENERATE = range(4)
PATH_NARROW, PATH_WAVE, PATH_BLOCK = range(3)
MAX_OBS = 1024


class IbaRefreshKeyframe(C.Structure):
    _fields_ = [("frame", C.c_int32), ("n_levels", C.c_int32), ("Tcw12", C.c_void_p), ("scale_factors", C.c_void_p), ("bad", C.c_int32), ("reserved", C.c_int32)]


class IbaRefreshOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("keep_stages", C.c_int32)]


class IbaRefreshCounts(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("status", C.c_int32 * 3), ("desc_state", C.c_int32 * 3), ("geo_state", C.c_int32 * 4), ("n_desc_changed", C.c_int32),
                ("path", C.c_int32 * 3), ("n_rows", C.c_int32)]


def _lib():
    L = load_library()
    L.iba_refresh_last_error.restype = C.c_char_p
    L.iba_refresh_last_error.argtypes = []
    L.iba_default_refresh_options.argtypes = [C.c_void_p]
    head = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p]
    L.iba_refresh.argtypes = head + [C.c_int, C.c_void_p]
    L.iba_debug_refresh_host.argtypes = head + [C.c_void_p]
    L.iba_refreshed_free.argtypes = [C.c_void_p]
    L.iba_refreshed_free.restype = None
    L.iba_refreshed_n.argtypes = [C.c_void_p]
    L.iba_refreshed_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.iba_refreshed_read.argtypes = [C.c_void_p] * 11
    L.iba_refreshed_medians.argtypes = [C.c_void_p] * 3
    L.iba_refresh_observations.argtypes = [C.c_void_p] * 4
    L.iba_refresh_store.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    L.iba_debug_refresh_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_refresh_last_error")


def refresh_options(**fields):
    """iba_default_refresh_options with fields overridden"""
    L = _lib()
    return options_from(IbaRefreshOptions, L.iba_default_refresh_options, L.iba_refresh_last_error, **fields)


def keyframe(frame, Tcw, scale_factors, bad=False):
    """an IbaRefreshKeyframe over copies of the arrays (kept alive by the struct): Tcw [3, 4] or [4, 4] f32"""
    k = IbaRefreshKeyframe()
    k._keep = (np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12]).copy(), np.ascontiguousarray(scale_factors, np.float32).reshape(-1).copy())
    k.frame, k.n_levels, k.bad = int(frame), len(k._keep[1]), int(bool(bad))
    k.Tcw12, k.scale_factors = k._keep[0].ctypes.data, k._keep[1].ctypes.data
    return k


def observations(fmap):
    """iba_refresh_observations over a fuse.FuseMap -> (obs_off [P + 1], obs_keyframe, obs_keypoint) i32"""
    L = _lib()
    off, kf, kp = np.zeros(fmap.P + 1, np.int32), np.zeros(max(len(fmap.holder), 1), np.int32), np.zeros(max(len(fmap.holder), 1), np.int32)
    m = fmap.struct()
    st = L.iba_refresh_observations(C.addressof(m), _p(off), _p(kf), _p(kp))
    if st != 0:
        _raise(L, st)
    return off, kf[:off[-1]].copy(), kp[:off[-1]].copy()


class Refreshed(Result):
    """iba_refreshed wrapper: the results of one iba_refresh; close() it"""
    FREE, LAST_ERROR = "iba_refreshed_free", "iba_refresh_last_error"

    def __len__(self):
        return int(self.lib.iba_refreshed_n(self.p))

    @property
    def stage_ms(self):
        """iba_debug_refresh_stage_ms: (narrow, wave, block) in ms; zeros unless IBA_REFRESH_TIMING was set"""
        ms = np.zeros(3, np.float32)
        self._chk(self.lib.iba_debug_refresh_stage_ms(self.p, _p(ms)))
        return ms

    def counts(self):
        """-> dict: n_points, status [3], desc_state [3], geo_state [4], n_desc_changed, path [3], n_rows"""
        c = IbaRefreshCounts()
        self._chk(self.lib.iba_refreshed_counts(self.p, C.addressof(c)))
        return {"n_points": c.n_points, "status": np.array(c.status[:], np.int32), "desc_state": np.array(c.desc_state[:], np.int32), "geo_state": np.array(c.geo_state[:], np.int32),
                "n_desc_changed": c.n_desc_changed, "path": np.array(c.path[:], np.int32), "n_rows": c.n_rows}

    def read(self):
        """-> dict per listed point: status, desc_state, geo_state u8, best_obs, best_median, n_desc i32, normal [n, 3], min_dist, max_dist f32, desc [n, 32] u8"""
        n = len(self)
        d = {"status": np.zeros(n, np.uint8), "desc_state": np.zeros(n, np.uint8), "geo_state": np.zeros(n, np.uint8), "best_obs": np.zeros(n, np.int32),
             "best_median": np.zeros(n, np.int32), "n_desc": np.zeros(n, np.int32), "normal": np.zeros((n, 3), np.float32), "min_dist": np.zeros(n, np.float32),
             "max_dist": np.zeros(n, np.float32), "desc": np.zeros((n, 32), np.uint8)}
        self._chk(self.lib.iba_refreshed_read(self.p, *[_p(a) for a in d.values()]))
        return d

    def medians(self):
        """keep_stages -> (off [n + 1], median [n_rows]) i32: per listed point the median of every observation's row in list order, -1 for a bad keyframe's"""
        off, med = np.zeros(len(self) + 1, np.int32), np.zeros(self.counts()["n_rows"], np.int32)
        self._chk(self.lib.iba_refreshed_medians(self.p, _p(off), _p(med)))
        return off, med

    def store(self, normal, min_dist, max_dist, desc, descriptor_stale=None):
        """iba_refresh_store into the caller's C-contiguous arrays (normal [P, 3] f32, min_dist, max_dist [P] f32, desc [P, 32] u8, descriptor_stale [P] u8 or
        None), in place"""
        for a, t in ((normal, np.float32), (min_dist, np.float32), (max_dist, np.float32), (desc, np.uint8)):
            assert a.dtype == t and a.flags["C_CONTIGUOUS"]
        assert descriptor_stale is None or (descriptor_stale.dtype == np.uint8 and descriptor_stale.flags["C_CONTIGUOUS"])
        self._chk(self.lib.iba_refresh_store(self.p, C.c_int32(len(min_dist)), _p(normal), _p(min_dist), _p(max_dist), _p(desc), _p(descriptor_stale)))


def _call(frames, keyframes, table, point_bad, ref_keyframe, obs_off, obs_keyframe, obs_keypoint, points, opt, device, host, fields):
    L = _lib()
    o = refresh_options(**fields) if opt is None else opt
    fa = (IbaOrbFrame * max(len(frames), 1))()
    for i, f in enumerate(frames):
        C.memmove(C.addressof(fa[i]), C.addressof(f), C.sizeof(IbaOrbFrame))
    ka = (IbaRefreshKeyframe * max(len(keyframes), 1))()
    for i, k in enumerate(keyframes):
        C.memmove(C.addressof(ka[i]), C.addressof(k), C.sizeof(IbaRefreshKeyframe))
    pb = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8).reshape(-1)
    rk, off = np.ascontiguousarray(ref_keyframe, np.int32).reshape(-1), np.ascontiguousarray(obs_off, np.int32).reshape(-1)
    okf, okp = np.ascontiguousarray(obs_keyframe, np.int32).reshape(-1), np.ascontiguousarray(obs_keypoint, np.int32).reshape(-1)
    pl = None if points is None else np.ascontiguousarray(points, np.int32).reshape(-1)
    n = table.n if pl is None else len(pl)
    data = lambda a: _p(a) if a is not None and len(a) else None
    p = C.c_void_p(None)
    head = [C.addressof(fa), C.c_int32(len(frames)), C.addressof(ka), C.c_int32(len(keyframes)), C.addressof(table), data(pb), data(rk), _p(off), data(okf), data(okp),
            None if pl is None else (_p(pl) if len(pl) else _p(np.zeros(1, np.int32))), C.c_int32(n), C.addressof(o)]
    st = L.iba_debug_refresh_host(*head, C.addressof(p)) if host else L.iba_refresh(*head, C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return Refreshed(L, p)


def refresh(frames, keyframes, table, point_bad, ref_keyframe, obs_off, obs_keyframe, obs_keypoint, points=None, opt=None, device=0, **fields):
    """iba_refresh: frames = a list of IbaOrbFrame, keyframes = a list of IbaRefreshKeyframe (keyframe()), table = map_match.points(), point_bad [P] u8 or
    None, ref_keyframe [P] i32, the observations as CSR arrays, points = the listed points or None (all P in order) -> Refreshed.
    opt = an IbaRefreshOptions, or fields of one over the defaults."""
    return _call(frames, keyframes, table, point_bad, ref_keyframe, obs_off, obs_keyframe, obs_keypoint, points, opt, device, False, fields)


def refresh_host(frames, keyframes, table, point_bad, ref_keyframe, obs_off, obs_keyframe, obs_keypoint, points=None, opt=None, **fields):
    """iba_debug_refresh_host: the same call through the host restatement of the rules, no device"""
    return _call(frames, keyframes, table, point_bad, ref_keyframe, obs_off, obs_keyframe, obs_keypoint, points, opt, 0, True, fields)
