"""ctypes mirror of the Sim3 RANSAC between two keyframes (include/iba_mi355x.h, iba_sim3*; csrc/iba_sim3.hip): jobs and options, the batch call on the
device or through the host restatement, the result object with its accessors, and the host-only helpers. The point table is map_match.points() (or
table() here, which fills what the unit does not read), the map of correspondences() a fuse.FuseMap. Plumbing only: nothing is computed here."""
import ctypes as C
from functools import partial

import numpy as np

from . import load_library
from ._percall import Result, options_from, ptr as _p, raise_last
from .map_match import points as _points

OK, NO_MORE, TOO_FEW = range(3)
MAX_ITERATIONS, MAX_EVENTS, TILE = 4096, 16, 256


class IbaSim3Job(C.Structure):
    _fields_ = [("Tcw12_1", C.c_void_p), ("Tcw12_2", C.c_void_p), ("point1", C.c_void_p), ("point2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("sets", C.c_void_p), ("n", C.c_int32), ("reserved", C.c_int32), ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float)]


class IbaSim3Options(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("min_inliers", C.c_int32), ("probability", C.c_double), ("max_iterations", C.c_int32), ("fix_scale", C.c_int32),
                ("max_events", C.c_int32), ("keep_stages", C.c_int32)]


class IbaSim3Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n", C.c_int32), ("iterations", C.c_int32), ("n_events", C.c_int32), ("n_listed", C.c_int32), ("best_it", C.c_int32),
                ("best_inliers", C.c_int32), ("sweep_cap_hits", C.c_int32)]


def _lib():
    L = load_library()
    L.iba_sim3_last_error.restype = C.c_char_p
    L.iba_sim3_last_error.argtypes = []
    L.iba_default_sim3_options.argtypes = [C.c_void_p]
    L.iba_sim3_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p]
    L.iba_debug_sim3_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_sim3_free.argtypes = [C.c_void_p]
    L.iba_sim3_free.restype = None
    L.iba_sim3_n_jobs.argtypes = [C.c_void_p]
    L.iba_sim3_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_sim3_counts.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.iba_sim3_event.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    L.iba_sim3_best.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    L.iba_sim3_iterations.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    L.iba_sim3_correspondences.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32] + [C.c_void_p] * 6
    L.iba_sim3_sets.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.c_void_p]
    L.iba_sim3_budget.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    L.iba_sim3_iterate.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iba_sim3_compose.argtypes = [C.c_float] + [C.c_void_p] * 6
    L.iba_debug_sim3_chunks.argtypes = [C.c_void_p]
    L.iba_debug_sim3_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
    return L


_raise = partial(raise_last, "iba_sim3_last_error")


def sim3_options(**fields):
    """iba_default_sim3_options with fields overridden"""
    L = _lib()
    return options_from(IbaSim3Options, L.iba_default_sim3_options, L.iba_sim3_last_error, **fields)


def table(xyz):
    """an IbaMapPoints of which only xyz is meaningful (the unit reads nothing else): xyz [P, 3] f32"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    P = len(xyz)
    return _points(xyz, np.zeros((P, 3), np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros((P, 32), np.uint8))


def job(Tcw1, Tcw2, K1, K2, point1, point2, max_err1, max_err2, sets):
    """an IbaSim3Job over copies of the arrays (kept alive by the struct): Tcw [3, 4] or [4, 4] f32, K = (fx, fy, cx, cy), point1, point2 [n] i32,
    max_err1, max_err2 [n] f32, sets [max_iterations, 3] i32 or None"""
    j = IbaSim3Job()
    keep = [np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1)[:12]).copy() for T in (Tcw1, Tcw2)]
    keep += [np.ascontiguousarray(a, np.int32).reshape(-1).copy() for a in (point1, point2)]
    keep += [np.ascontiguousarray(a, np.float32).reshape(-1).copy() for a in (max_err1, max_err2)]
    keep.append(None if sets is None else np.ascontiguousarray(sets, np.int32).reshape(-1).copy())
    j._keep = keep
    n = len(keep[2])
    assert all(len(a) == n for a in keep[2:6])
    j.Tcw12_1, j.Tcw12_2 = keep[0].ctypes.data, keep[1].ctypes.data
    j.point1, j.point2, j.max_err1, j.max_err2 = (a.ctypes.data if n else None for a in keep[2:6])
    j.sets = None if keep[6] is None or not len(keep[6]) else keep[6].ctypes.data
    j.n = n
    (j.fx1, j.fy1, j.cx1, j.cy1), (j.fx2, j.fy2, j.cx2, j.cy2) = (float(x) for x in K1), (float(x) for x in K2)
    return j


def sets(N, iterations, seed=0):
    """iba_sim3_sets -> [iterations, 3] i32"""
    L = _lib()
    out = np.zeros((max(iterations, 1), 3), np.int32)
    st = L.iba_sim3_sets(C.c_int32(N), C.c_int32(iterations), C.c_uint64(seed), _p(out))
    if st != 0:
        _raise(L, st)
    return out


def budget(N, opt=None, **fields):
    """iba_sim3_budget -> the iterations of a job with N correspondences"""
    L = _lib()
    o = sim3_options(**fields) if opt is None else opt
    it = C.c_int32(0)
    st = L.iba_sim3_budget(C.c_int32(N), C.addressof(o), C.addressof(it))
    if st != 0:
        _raise(L, st)
    return it.value


def correspondences(fmap, kf1, kf2, matches12, octave1, octave2, level_sigma2_1, level_sigma2_2):
    """iba_sim3_correspondences over a fuse.FuseMap -> dict: index1, point1, point2 i32, max_err1, max_err2 f32"""
    L = _lib()
    m12, o1, o2 = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (matches12, octave1, octave2))
    s1, s2 = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (level_sigma2_1, level_sigma2_2))
    cap = max(len(m12), 1)
    d = {"index1": np.zeros(cap, np.int32), "point1": np.zeros(cap, np.int32), "point2": np.zeros(cap, np.int32), "max_err1": np.zeros(cap, np.float32),
         "max_err2": np.zeros(cap, np.float32)}
    n = C.c_int32(0)
    m = fmap.struct()
    st = L.iba_sim3_correspondences(C.addressof(m), C.c_int32(kf1), C.c_int32(kf2), _p(m12), _p(o1), _p(o2), _p(s1), _p(s2), C.c_int32(len(s1)), C.c_int32(len(s2)),
                                    *[_p(a) for a in d.values()], C.addressof(n))
    if st != 0:
        _raise(L, st)
    return {k: a[:n.value].copy() for k, a in d.items()}


def compose(s, R, t, Tmw):
    """iba_sim3_compose -> (s, R [3, 3], t [3]) f64"""
    L = _lib()
    Ra, ta = np.ascontiguousarray(R, np.float32).reshape(-1), np.ascontiguousarray(t, np.float32).reshape(-1)
    Tm = np.ascontiguousarray(np.asarray(Tmw, np.float32).reshape(-1)[:12])
    so, Ro, to = C.c_double(0), np.zeros(9, np.float64), np.zeros(3, np.float64)
    st = L.iba_sim3_compose(C.c_float(s), _p(Ra), _p(ta), _p(Tm), C.addressof(so), _p(Ro), _p(to))
    if st != 0:
        _raise(L, st)
    return so.value, Ro.reshape(3, 3), to


class Sim3Batch(Result):
    """iba_sim3_batch wrapper: the results of the jobs of one iba_sim3_solve; close() it"""
    FREE, LAST_ERROR = "iba_sim3_free", "iba_sim3_last_error"

    def __len__(self):
        return int(self.lib.iba_sim3_n_jobs(self.p))

    @property
    def n_chunks(self):
        return int(self.lib.iba_debug_sim3_chunks(self.p))

    @property
    def stage_ms(self):
        """iba_debug_sim3_stage_ms: (preparation, hypotheses, count, selection, flags) in ms; zeros unless IBA_SIM3_TIMING was set"""
        ms = np.zeros(5, np.float32)
        self._chk(self.lib.iba_debug_sim3_stage_ms(self.p, _p(ms)))
        return ms

    def read(self, job):
        """-> dict of iba_sim3_result's fields"""
        r = IbaSim3Result()
        self._chk(self.lib.iba_sim3_read(self.p, C.c_int32(job), C.addressof(r)))
        return {k: getattr(r, k) for k, _ in IbaSim3Result._fields_}

    def counts(self, job):
        """-> [iterations] i32: the inliers of every iteration"""
        c = np.zeros(self.read(job)["iterations"], np.int32)
        self._chk(self.lib.iba_sim3_counts(self.p, C.c_int32(job), _p(c)))
        return c

    def _hyp(self, fn, job, *head):
        it, n = C.c_int32(0), C.c_int32(0)
        s, R, t, inl = C.c_float(0), np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(self.read(job)["n"], np.uint8)
        self._chk(fn(self.p, C.c_int32(job), *head, C.addressof(it), C.addressof(n), C.addressof(s), _p(R), _p(t), _p(inl)))
        return {"iteration": it.value, "n_inliers": n.value, "s": np.float32(s.value), "R": R, "t": t, "inlier": inl}

    def event(self, job, k):
        """the k-th event -> dict: iteration, n_inliers, s, R [9], t [3] f32, inlier [N] u8"""
        return self._hyp(self.lib.iba_sim3_event, job, C.c_int32(k))

    def best(self, job):
        """the best after the last iteration, as event()"""
        return self._hyp(self.lib.iba_sim3_best, job)

    def iterations(self, job):
        """keep_stages -> dict: s [I], R [I, 9], t [I, 3] f32, inlier [I, N] u8"""
        r = self.read(job)
        I, N = r["iterations"], r["n"]
        d = {"s": np.zeros(I, np.float32), "R": np.zeros((I, 9), np.float32), "t": np.zeros((I, 3), np.float32), "inlier": np.zeros((I, N), np.uint8)}
        self._chk(self.lib.iba_sim3_iterations(self.p, C.c_int32(job), *[_p(a) for a in d.values()]))
        return d

    def iterate(self, job, from_it, n):
        """iba_sim3_iterate: one iterate(n) of the reference -> (next_it, event or -1, no_more)"""
        nx, ev, nm = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.iba_sim3_iterate(self.p, C.c_int32(job), C.c_int32(from_it), C.c_int32(n), C.addressof(nx), C.addressof(ev), C.addressof(nm)))
        return nx.value, ev.value, bool(nm.value)


def _call(tb, jobs, opt, device, host, fields):
    L = _lib()
    o = sim3_options(**fields) if opt is None else opt
    ja = (IbaSim3Job * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        C.memmove(C.addressof(ja[i]), C.addressof(j), C.sizeof(IbaSim3Job))
    p = C.c_void_p(None)
    head = [C.addressof(tb), C.addressof(ja), C.c_int32(len(jobs)), C.addressof(o)]
    st = L.iba_debug_sim3_host(*head, C.addressof(p)) if host else L.iba_sim3_solve(*head, C.c_int(device), C.addressof(p))
    if st != 0:
        _raise(L, st)
    return Sim3Batch(L, p)


def solve(tb, jobs, opt=None, device=0, **fields):
    """iba_sim3_solve: tb = map_match.points() or table(), jobs = a list of IbaSim3Job (job()) -> Sim3Batch. opt = an IbaSim3Options, or fields of one
    over the defaults."""
    return _call(tb, jobs, opt, device, False, fields)


def solve_host(tb, jobs, opt=None, **fields):
    """iba_debug_sim3_host: the same call through the host restatement of the rules, no device"""
    return _call(tb, jobs, opt, 0, True, fields)
