"""ctypes mirror of the ORB feature extraction (include/iba_mi355x.h, iba_orb_*; csrc/iba_orb.hip): the options, the batch call, the result object
with its stage accessors, and the two host-only pure functions (plan, distribute). Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last


class IbaOrbImage(C.Structure):
    _fields_ = [("gray", C.c_void_p), ("W", C.c_int32), ("H", C.c_int32), ("stride", C.c_int64)]


class IbaOrbOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32), ("ini_th_fast", C.c_int32),
                ("min_th_fast", C.c_int32), ("keep_stages", C.c_int32), ("reserved", C.c_int32), ("pattern", C.c_void_p)]


def _lib():
    L = load_library()
    L.iba_orb_last_error.restype = C.c_char_p
    L.iba_orb_last_error.argtypes = []
    L.iba_default_orb_options.argtypes = [C.POINTER(IbaOrbOptions)]
    L.iba_orb_extract.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_orb_free.argtypes = [C.c_void_p]
    L.iba_orb_free.restype = None
    L.iba_orb_n_images.argtypes = [C.c_void_p]
    L.iba_orb_counts.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_orb_read.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    L.iba_orb_level.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.iba_orb_scores.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.iba_orb_candidates.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_orb_plan.argtypes = [C.c_int32, C.c_int32, C.c_void_p] + [C.c_void_p] * 5
    L.iba_orb_distribute.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_debug_orb_atan2.argtypes = [C.c_float, C.c_float]
    L.iba_debug_orb_atan2.restype = C.c_float
    L.iba_debug_orb_sincos.argtypes = [C.c_float, C.c_void_p, C.c_void_p]
    L.iba_debug_orb_stub.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.iba_debug_orb_chunks.argtypes = [C.c_void_p]
    L.iba_debug_orb_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    L.iba_debug_orb_describe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_orb_last_error")


def orb_options(pattern=None, **fields):
    """iba_default_orb_options with fields overridden. pattern: int8 [256, 4] (x0 y0 x1 y1 per test); the returned struct keeps the array alive."""
    L = _lib()
    o = options_from(IbaOrbOptions, L.iba_default_orb_options, L.iba_orb_last_error, **fields)
    if pattern is not None:
        o._pattern = np.ascontiguousarray(pattern, np.int8).reshape(256, 4)
        o.pattern = o._pattern.ctypes.data
    return o


def plan(W, H, opt):
    """iba_orb_plan (host only) -> dict: level_wh [L, 2], features_per_level [L], cells [L, 4] (nCols nRows wCell hCell), n_ini [L], umax [16]"""
    L = _lib()
    n = min(max(int(opt.n_levels), 1), 16) if opt is not None else 1   # (outside 1..16 the call refuses and writes nothing)
    out = {"level_wh": np.zeros((n, 2), np.int32), "features_per_level": np.zeros(n, np.int32), "cells": np.zeros((n, 4), np.int32),
           "n_ini": np.zeros(n, np.int32), "umax": np.zeros(16, np.int32)}
    st = L.iba_orb_plan(C.c_int32(W), C.c_int32(H), None if opt is None else C.addressof(opt), _p(out["level_wh"]), _p(out["features_per_level"]),
                        _p(out["cells"]), _p(out["n_ini"]), _p(out["umax"]))
    if st != 0:
        _raise(L, st)
    return out


def distribute(xy, score, width, height, N):
    """iba_orb_distribute (host only): xy int32 [n, 2], score int32 [n] -> chosen candidate indices in the order of the node list"""
    L = _lib()
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    sc = np.ascontiguousarray(score, np.int32).reshape(-1)
    assert len(xy) == len(sc)
    chosen, n = np.zeros(max(len(sc), 1), np.int32), C.c_int32(0)
    st = L.iba_orb_distribute(_p(xy), _p(sc), C.c_int32(len(sc)), C.c_int32(width), C.c_int32(height), C.c_int32(N), _p(chosen), C.addressof(n))
    if st != 0:
        _raise(L, st)
    return chosen[:n.value].copy()


def atan2_deg(y, x):
    """iba_debug_orb_atan2 (host only): O7's polynomial"""
    return float(_lib().iba_debug_orb_atan2(C.c_float(y), C.c_float(x)))


def sincos(angle_deg):
    """iba_debug_orb_sincos (host only) -> (a, b) float32 as the descriptor uses them, (cos, sin) float64 before the rounding"""
    L = _lib()
    ab, cs = np.zeros(2, np.float32), np.zeros(2, np.float64)
    st = L.iba_debug_orb_sincos(C.c_float(angle_deg), _p(ab), _p(cs))
    if st != 0:
        _raise(L, st)
    return ab, cs


def describe(gray, xy, angle, pattern, device=0):
    """iba_debug_orb_describe: O8 and O9 alone on one image -> (blurred [H, W] uint8, desc [n, 32] uint8)"""
    L = _lib()
    img = np.ascontiguousarray(gray, np.uint8)
    H, W = img.shape
    pts = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    ang = np.ascontiguousarray(angle, np.float32).reshape(-1)
    pat = np.ascontiguousarray(pattern, np.int8).reshape(256, 4)
    blurred, desc = np.zeros((H, W), np.uint8), np.zeros((len(ang), 32), np.uint8)
    st = L.iba_debug_orb_describe(_p(img), C.c_int32(W), C.c_int32(H), _p(pts), _p(ang), C.c_int32(len(ang)), _p(pat), C.c_int(device), _p(blurred), _p(desc))
    if st != 0:
        _raise(L, st)
    return blurred, desc


class OrbFeatures(Result):
    """iba_orb_features wrapper: the keypoints and descriptors of the images of one iba_orb_extract; close() it"""
    FREE, LAST_ERROR = "iba_orb_free", "iba_orb_last_error"

    def __init__(self, lib, p, n_levels):
        super().__init__(lib, p)
        self.n_levels = n_levels

    @classmethod
    def stub(cls, n_images, n_levels=8, keep_stages=0):
        """iba_debug_orb_stub (host only): empty images without device buffers"""
        L = _lib()
        p = C.c_void_p(None)
        st = L.iba_debug_orb_stub(C.c_int32(n_images), C.c_int32(n_levels), C.c_int32(keep_stages), C.addressof(p))
        if st != 0:
            _raise(L, st)
        return cls(L, p, n_levels)

    def __len__(self):
        return int(self.lib.iba_orb_n_images(self.p))

    @property
    def n_chunks(self):
        return int(self.lib.iba_debug_orb_chunks(self.p))

    @property
    def stage_ms(self):
        """iba_debug_orb_stage_ms: (resize, score, cell, host distribution with both copies, orientation, blur, descriptor) in ms; zeros unless IBA_ORB_TIMING was set"""
        ms = np.zeros(7, np.float32)
        self._chk(self.lib.iba_debug_orb_stage_ms(self.p, _p(ms)))
        return ms

    def counts(self, image):
        """-> dict: n_keypoints, per_level, candidates_per_level, fallback_cells_per_level"""
        n = C.c_int32(0)
        per, cand, fb = (np.zeros(self.n_levels, np.int32) for _ in range(3))
        self._chk(self.lib.iba_orb_counts(self.p, C.c_int32(image), C.addressof(n), _p(per), _p(cand), _p(fb)))
        return {"n_keypoints": n.value, "per_level": per, "candidates_per_level": cand, "fallback_cells_per_level": fb}

    def read(self, image):
        """-> dict: xy [n, 2] f32, angle, response, size [n] f32, octave [n] i32, desc [n, 32] u8"""
        n = self.counts(image)["n_keypoints"]
        out = {"xy": np.zeros((n, 2), np.float32), "angle": np.zeros(n, np.float32), "response": np.zeros(n, np.float32), "octave": np.zeros(n, np.int32),
               "size": np.zeros(n, np.float32), "desc": np.zeros((n, 32), np.uint8)}
        self._chk(self.lib.iba_orb_read(self.p, C.c_int32(image), *[_p(out[k]) for k in ("xy", "angle", "response", "octave", "size", "desc")]))
        return out

    def level(self, image, level, wh, blurred=False):
        """a pyramid level (or its blurred copy) [Hl, Wl] uint8; wh = the level's (Wl, Hl) of plan()"""
        out = np.zeros((int(wh[1]), int(wh[0])), np.uint8)
        self._chk(self.lib.iba_orb_level(self.p, C.c_int32(image), C.c_int32(level), C.c_int32(1 if blurred else 0), _p(out)))
        return out

    def scores(self, image, level, wh):
        out = np.zeros((int(wh[1]), int(wh[0])), np.uint8)
        self._chk(self.lib.iba_orb_scores(self.p, C.c_int32(image), C.c_int32(level), _p(out)))
        return out

    def candidates(self, image, level):
        """-> (xy [n, 2] int32 relative to minB, score [n] int32) in O5's order"""
        n = int(self.counts(image)["candidates_per_level"][level]) if 0 <= level < self.n_levels else 0
        xy, sc = np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
        self._chk(self.lib.iba_orb_candidates(self.p, C.c_int32(image), C.c_int32(level), _p(xy), _p(sc)))
        return xy, sc


def extract(images, opt=None, device=0, pattern=None, **fields):
    """iba_orb_extract: images = a list of uint8 [H, W] arrays (any row stride of whole bytes) -> OrbFeatures. opt = an IbaOrbOptions, or fields of one
    over the defaults with pattern."""
    L = _lib()
    o = orb_options(pattern, **fields) if opt is None else opt
    keep = []
    arr = (IbaOrbImage * max(len(images), 1))()
    for i, im in enumerate(images):
        a = np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 2 or a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a, np.uint8)
        keep.append(a)
        arr[i].gray, arr[i].W, arr[i].H, arr[i].stride = a.ctypes.data, a.shape[1], a.shape[0], a.strides[0]
    p = C.c_void_p(None)
    st = L.iba_orb_extract(C.addressof(arr), C.c_int32(len(images)), C.addressof(o), C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return OrbFeatures(L, p, int(o.n_levels))
