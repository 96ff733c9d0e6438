"""A stand-in for the shared library behind `IntegratorCache._L` / `ScvxBatch._L` that records the C traffic of the Python binding.

It needs neither libscvx_hip.so nor a device.  `Recorder` answers every name of `_lib.SIGNATURES` with a function that checks the
argument count against SIGNATURES and the header, passes every argument through its argtype's `from_param` (a wrong ctypes kind fails
here, as it would at the real call), writes one line and returns 0.  A line holds the entry point's name and, per argument, the header's
parameter name with: a scalar by value; a struct passed by reference by its bytes; an array (the `_arr` back-reference numpy's `data_as`
keeps on the pointer) by dtype and shape, and -- where include/scvx.h declares the parameter `const` -- the CRC-32 of its bytes.  Every
array argument that is NOT const is then filled with a fixed arithmetic pattern, so that a later call fed from an earlier call's output
sees the same values on every run.  `Unreachable` is the stand-in of the refusal cases: it fails when the library is reached.

`make_cache` builds the plain object the module-level calls take for a cache; `ScvxBatch(cache, B)` works on top of it.
"""
import ctypes as C
import functools
import os
import re
import zlib
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_INTS = (C.c_int, C.c_uint, C.c_int32, C.c_int64, C.c_size_t)
_FLOATS = (C.c_double, C.c_float)


def header_params():
    """{function: [(declared const, parameter name), ...]} of every function include/scvx.h declares, the handle included"""
    src = open(os.path.join(ROOT, "include", "scvx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for m in re.finditer(r"\b(scvx_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", src):
        ps = [" ".join(p.split()) for p in m.group(2).split(",")]
        ps = [p for p in ps if p not in ("", "void")]
        names = [re.search(r"(\w+)\s*(?:\[\w*\])?$", p) for p in ps]
        out[m.group(1)] = [(p.startswith("const "), n.group(1) if n else "arg%d" % i) for i, (p, n) in enumerate(zip(ps, names))]
    return out


def pattern(shape, step=1, dtype=np.float64):
    """a dyadic arithmetic pattern: ((i * step) mod 13 + 1) / 16 over the flattened index i"""
    n = int(np.prod(shape))
    v = ((np.arange(n, dtype=np.int64) * int(step)) % 13 + 1)
    return (v / 16.0).reshape(shape) if np.issubdtype(np.dtype(dtype), np.floating) else (v % 3).astype(dtype).reshape(shape)


class Recorder:
    def __init__(self):
        from successiveconvexification_amd import _lib
        self.lines = []
        self._sig = _lib.SIGNATURES
        self._par = header_params()
        assert set(self._par) == set(self._sig), set(self._par) ^ set(self._sig)

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._sig:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    @staticmethod
    def _show(a, t, const):
        if a is None:
            return "NULL"
        arr = getattr(a, "_arr", None)
        if arr is not None:
            s = "%s%s" % (arr.dtype.str, list(arr.shape))
            return s + (" crc=%08x" % zlib.crc32(np.ascontiguousarray(arr).tobytes()) if const else "")
        obj = getattr(a, "_obj", None)
        if obj is not None:
            return "&%s{%s}" % (type(obj).__name__, bytes(obj).hex()) if isinstance(obj, C.Structure) else "&" + type(obj).__name__
        if isinstance(a, C.c_void_p):
            return "handle"
        if t in _INTS:
            return "%d" % int(a)
        if t in _FLOATS:
            return repr(float(a))
        raise AssertionError("an argument the recorder cannot describe: %r for %r" % (a, t))

    def _call(self, name, *args):
        argtypes, params = self._sig[name][1], self._par[name]
        assert len(args) == len(argtypes) == len(params), (name, len(args), len(argtypes), len(params))
        shown = []
        for a, t, (const, pname) in zip(args, argtypes, params):
            t.from_param(a)
            shown.append("%s=%s" % (pname, self._show(a, t, const)))
        self.lines.append("%s(%s)" % (name, ", ".join(shown)))
        for a, (const, _) in zip(args, params):
            arr = getattr(a, "_arr", None)
            if arr is not None and not const:
                arr[...] = pattern(arr.shape, dtype=arr.dtype)
        return 0


class Unreachable:
    """the stand-in of the refusal cases: looking an entry point up is allowed (Python evaluates `L.name` before the arguments of
    `L.name(...)`, and building those may still refuse), calling it is not"""

    def __getattr__(self, name):
        def reached(*args):
            raise AssertionError("the library must not be reached: %s" % name)
        return reached


def make_cache(L, nu, aero, K=3, npts=4):
    """the plain object that stands for an IntegratorCache: handle, _L, nu, np, npts and problem (K, aero and the constants
    montecarlo.margins_from_quantiles reads)"""
    from successiveconvexification_amd.defns import AtmosphericData
    z = np.zeros((2, 2))
    prob = SimpleNamespace(K=K, aero=AtmosphericData(z, z, z) if aero else None, Tmin=0.25, Tmax=2.0, mwet=1.0, mdry=0.5, omMax=0.5,
                           gammaGs=20.0, thetaMax=90.0)
    return SimpleNamespace(handle=C.c_void_p(1), _L=L, nu=nu, np=15 + 2 * nu, npts=npts, problem=prob)
