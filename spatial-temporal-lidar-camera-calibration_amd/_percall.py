"""What the ctypes mirrors of the per-call units share (project, orb, orb_match, twoview, pose, bundle; csrc/iba_call.hpp is the native side): the array
pointer, the error of a failed call, the result object's ownership and the options-with-overrides pattern. Plumbing only."""
import ctypes as C

from . import IbaError


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raise_last(last_error, lib, st):
    """IbaError with the unit's message: last_error = the name of its iba_*_last_error"""
    raise IbaError(st, getattr(lib, last_error)().decode())


class Result:
    """a result object of the library: lib, the pointer p, and the names of the unit's free and last-error functions; close() it"""
    FREE = LAST_ERROR = None

    def __init__(self, lib, p):
        self.lib, self.p = lib, p

    def _chk(self, st):
        if st != 0:
            raise_last(self.LAST_ERROR, self.lib, st)

    def close(self):
        if getattr(self, "p", None) and self.p.value:
            getattr(self.lib, self.FREE)(self.p)
            self.p = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def options_from(StructType, default_fn, last_error_fn, **fields):
    """the unit's default options with fields overridden"""
    o = StructType()
    st = default_fn(C.byref(o))
    if st != 0:
        raise IbaError(st, last_error_fn().decode())
    for k, v in fields.items():
        if k not in dict(StructType._fields_):
            raise AttributeError(k)
        setattr(o, k, v)
    return o
