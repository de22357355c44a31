"""ctypes mirror of the scan-to-image projection (include/iba_mi355x.h, iba_project_* / iba_projection_*; csrc/iba_project.hip): the options, the run
on a handle, and the result object whose accessors copy one job's product down. Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last

IN_FRONT, INSIDE, VISIBLE = 1, 2, 4


class IbaProjectOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("splat", C.c_int32), ("occlusion_tol", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
                ("v_focal_is_fx", C.c_int32), ("reserved", C.c_int32), ("camera", C.c_double * 6), ("z_near", C.c_double), ("z_far", C.c_double)]


class IbaProjectCounts(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_points", "n_skipped", "n_in_front", "n_inside", "n_visible", "n_pixels")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def _lib():
    L = load_library()
    L.iba_project_last_error.restype = C.c_char_p
    L.iba_project_last_error.argtypes = []
    L.iba_default_project_options.argtypes = [C.POINTER(IbaProjectOptions)]
    L.iba_project_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(IbaProjectOptions), C.POINTER(C.c_void_p)]
    L.iba_projection_free.argtypes = [C.c_void_p]
    L.iba_projection_free.restype = None
    L.iba_projection_n_jobs.argtypes = [C.c_void_p]
    L.iba_projection_size.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.iba_projection_pose.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_projection_counts.argtypes = [C.c_void_p, C.c_int32, C.POINTER(IbaProjectCounts)]
    L.iba_projection_depth.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_projection_index.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_projection_points.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_projection_colorize.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_projection_overlay.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_project_gradient.argtypes = [C.c_double, C.c_void_p]
    L.iba_debug_project_validate.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_debug_project_stub.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.iba_debug_projection_chunks.argtypes = [C.c_void_p]
    return L


_raise = partial(raise_last, "iba_project_last_error")


def project_options(**fields):
    """iba_default_project_options with fields overridden; camera takes six numbers (fx, fy, cx, cy, W, H)"""
    L = _lib()
    camera = fields.pop("camera", None)
    o = options_from(IbaProjectOptions, L.iba_default_project_options, L.iba_project_last_error, **fields)
    if camera is not None:
        o.camera[:] = [float(x) for x in np.asarray(camera, np.float64).reshape(6)]
    return o


def gradient(zn):
    """iba_project_gradient (host only): the overlay's palette at zn -> uint8 [3]"""
    L = _lib()
    rgb = np.zeros(3, np.uint8)
    st = L.iba_project_gradient(C.c_double(zn), _p(rgb))
    if st != 0:
        _raise(L, st)
    return rgb


def validate(n_frames, intrinsics6, x7, frames, J, opt):
    """iba_debug_project_validate (host only): the argument checks of iba_project_run on a stand-in for the handle; any argument may be None.
    Raises IbaError as run() would; returns None when the arguments are valid."""
    L = _lib()
    intr = None if intrinsics6 is None else np.ascontiguousarray(intrinsics6, np.float64)
    xs = None if x7 is None else np.ascontiguousarray(x7, np.float64)
    fr = None if frames is None else np.ascontiguousarray(frames, np.int32)
    st = L.iba_debug_project_validate(C.c_int32(n_frames), _p(intr), _p(xs), _p(fr), C.c_int32(J), None if opt is None else C.byref(opt))
    if st != 0:
        _raise(L, st)


class Projection(Result):
    """iba_projection wrapper: the products of the jobs of one iba_project_run, on the device until an accessor copies one job down; close() it"""
    FREE, LAST_ERROR = "iba_projection_free", "iba_project_last_error"

    @classmethod
    def stub(cls, n_jobs):
        """iba_debug_project_stub (host only): n_jobs empty jobs without device buffers"""
        L = _lib()
        p = C.c_void_p(None)
        st = L.iba_debug_project_stub(C.c_int32(n_jobs), C.byref(p))
        if st != 0:
            _raise(L, st)
        return cls(L, p)

    def __len__(self):
        return int(self.lib.iba_projection_n_jobs(self.p))

    @property
    def n_chunks(self):
        return int(self.lib.iba_debug_projection_chunks(self.p))

    @property
    def kernel_ms(self):
        """iba_debug_projection_kernel_ms: (splat, resolve, visible, last colourise, last overlay) in ms; zeros unless IBA_PROJECT_TIMING was set"""
        ms = np.zeros(5, np.float32)
        self.lib.iba_debug_projection_kernel_ms.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self.lib.iba_debug_projection_kernel_ms(self.p, _p(ms)))
        return ms

    def size(self, job):
        W, H = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.iba_projection_size(self.p, C.c_int32(job), C.byref(W), C.byref(H)))
        return W.value, H.value

    def pose(self, job):
        """R | t [3, 4] the device used"""
        out = np.zeros(12)
        self._chk(self.lib.iba_projection_pose(self.p, C.c_int32(job), _p(out)))
        return out.reshape(3, 4)

    def counts(self, job):
        c = IbaProjectCounts()
        self._chk(self.lib.iba_projection_counts(self.p, C.c_int32(job), C.byref(c)))
        return c.as_dict()

    def depth(self, job):
        W, H = self.size(job)
        out = np.zeros((H, W), np.float32)
        self._chk(self.lib.iba_projection_depth(self.p, C.c_int32(job), _p(out)))
        return out

    def index(self, job):
        W, H = self.size(job)
        out = np.zeros((H, W), np.uint32)
        self._chk(self.lib.iba_projection_index(self.p, C.c_int32(job), _p(out)))
        return out

    def points(self, job):
        """(uv [n, 2] float64, z [n] float32, flags [n] uint8) in the original order of the frame's scan"""
        n = self.counts(job)["n_points"]
        uv, z, fl = np.zeros((n, 2)), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        self._chk(self.lib.iba_projection_points(self.p, C.c_int32(job), _p(uv), _p(z), _p(fl)))
        return uv, z, fl

    def colorize(self, job, rgb):
        """rgb [H, W, 3] uint8 -> a colour per point [n, 3] uint8 (0 0 0 where the point is not VISIBLE)"""
        W, H = self.size(job)
        img = np.ascontiguousarray(rgb, np.uint8)
        assert img.shape == (H, W, 3)
        out = np.zeros((self.counts(job)["n_points"], 3), np.uint8)
        self._chk(self.lib.iba_projection_colorize(self.p, C.c_int32(job), _p(img), _p(out)))
        return out

    def overlay(self, job, rgb=None):
        """rgb [H, W, 3] uint8 or None (black) -> the image with the gradient's colour at every pixel that holds a point"""
        W, H = self.size(job)
        img = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
        assert img is None or img.shape == (H, W, 3)
        out = np.zeros((H, W, 3), np.uint8)
        self._chk(self.lib.iba_projection_overlay(self.p, C.c_int32(job), _p(img), _p(out)))
        return out


def run(handle, x7, frames, opt=None, **fields):
    """iba_project_run on an IbaHandle: x7 [J, 7], frames [J] local frames -> Projection. opt = an IbaProjectOptions, or fields of one over the defaults."""
    L = _lib()
    o = project_options(**fields) if opt is None else opt
    xs = np.ascontiguousarray(np.asarray(x7, np.float64).reshape(-1, 7))
    fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
    assert len(xs) == len(fr)
    p = C.c_void_p(None)
    st = L.iba_project_run(handle.h, _p(xs), _p(fr), C.c_int32(len(fr)), C.byref(o), C.byref(p))
    if st != 0:
        _raise(L, st)
    return Projection(L, p)
