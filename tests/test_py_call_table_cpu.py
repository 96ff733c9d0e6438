"""The call table of the Python binding (successiveconvexification_amd/_calls.py) against include/scvx.h and _lib.SIGNATURES, without a
shared library or a device: what makes filling a record by the header's parameter names sound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from py_call_recorder import Recorder, header_params
from test_py_call_traffic_cpu import FAMILIES


def _kind(argtype):
    if argtype in (C.c_int, C.c_uint):
        return "int"
    if argtype is C.c_double:
        return "double"
    if argtype is C.c_void_p:
        return "void pointer"
    return "struct pointer" if issubclass(argtype._type_, C.Structure) else "pointer to " + argtype._type_.__name__


def test_every_tuple_is_the_header_parameter_list():
    from successiveconvexification_amd import _calls
    hdr = header_params()
    for name, fields in _calls.TABLE.items():
        assert name in hdr, name
        assert hdr[name][0][1] in ("ctx", "b"), name                           # the leading handle
        assert tuple(n for _, n in hdr[name][1:]) == fields, (name, [n for _, n in hdr[name][1:]], fields)


def test_every_position_has_the_kind_the_binding_declares():
    """the dispatcher converts by _lib.SIGNATURES: its kind at every position is the kind the header declares there"""
    from successiveconvexification_amd import _calls, _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scvx.h")).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    for name, fields in _calls.TABLE.items():
        decl = re.search(r"\b%s\s*\(([^;{()]*)\)\s*;" % name, src).group(1).split(",")
        argtypes = _lib.SIGNATURES[name][1]
        assert len(decl) == len(argtypes) == len(fields) + 1, name
        assert argtypes[0] is C.c_void_p, name
        for d, t, field in zip(decl[1:], argtypes[1:], fields):
            d = " ".join(d.replace("const ", "").split())
            ctype = d[:d.rindex(field)].strip()
            want = {"int": "int", "unsigned": "int", "double": "double", "double *": "pointer to c_double", "int *": "pointer to c_int",
                    "void *": "void pointer", "scvx_mc_rng *": "struct pointer", "scvx_mc_vehicle *": "struct pointer"}[ctype]
            assert _kind(t) == want, (name, field, ctype, t)


def test_the_table_holds_every_host_and_batch_form_of_the_two_families():
    from successiveconvexification_amd import _calls
    declared = {n for n in header_params() if re.fullmatch(FAMILIES, n) and (n.endswith("_host") or n.startswith("scvx_batch_"))}
    assert declared == set(_calls.TABLE), declared ^ set(_calls.TABLE)
    assert len(declared) == 33


def test_the_dispatcher_lays_a_record_out_and_refuses_a_missing_field():
    from successiveconvexification_amd import _calls, _lib
    rec = Recorder()
    h = C.c_void_p(1)
    f = dict(handle=h, q14=np.ones(14), rNU=np.ones(3), qf14=np.ones(14), S0=np.zeros((2, 14, 14)), w14=None, nsigma=3, cap=0.25,
             which=np.int64(5), psig=None, extra="ignored")
    _calls.call(rec, h, "scvx_batch_margins_from_cov", f)
    assert rec.lines == ["scvx_batch_margins_from_cov(b=handle, q14=<f8[14] crc=%s, rNU=<f8[3] crc=%s, qf14=<f8[14] crc=%s, "
                         "S0=<f8[2, 14, 14] crc=%s, w14=NULL, nsigma=3.0, cap=0.25, which=5, psig=NULL)"
                         % tuple(re.findall(r"crc=(\w+)", rec.lines[0]))]
    del f["cap"]
    with pytest.raises(KeyError):
        _calls.call(rec, h, "scvx_batch_margins_from_cov", f)
    with pytest.raises(KeyError):
        _calls.call(rec, h, "scvx_batch_track_fly", f)                      # not one of the two families
    assert len(rec.lines) == 1

    class Failing:
        scvx_batch_margins_from_cov = staticmethod(lambda *a: -1)
    f["cap"] = 0.25
    seen = []
    orig, _lib.check = _lib.check, lambda hh, rc, what: seen.append((hh, rc, what))
    try:
        _calls.call(Failing, h, "scvx_batch_margins_from_cov", f)
    finally:
        _lib.check = orig
    assert seen == [(h, -1, "scvx_batch_margins_from_cov")]


def test_one_entry_point_per_record():
    from successiveconvexification_amd import _calls
    off = dict(veh=None, rng=None, nq=0, pathv=None)
    assert _calls.mc_entry(off) == "scvx_track_mc_f64_host" and _calls.mc_entry(dict(off, CN=1, q14=1)) == "scvx_batch_track_mc_nav"
    assert _calls.mc_entry(dict(off, pathv=np.zeros(1))) == "scvx_track_mc_q_f64_host" == _calls.mc_entry(dict(off, nq=2))
    assert _calls.mc_entry(dict(off, nq=2, rng=1, CN=1)) == "scvx_track_mc_nav_rng_f64_host"
    assert _calls.mc_entry(dict(off, nq=2, rng=1, veh=1, q14=1)) == "scvx_batch_track_mc_veh"
    assert {_calls.mc_entry(dict(off, **a, **b, **c)) for a in ({}, dict(CN=1)) for b in ({}, dict(q14=1))
            for c in ({}, dict(nq=1), dict(rng=1), dict(veh=1))} == {n for n in _calls.TABLE if "track_mc" in n}
    ctx = dict(psig=None)
    got = {_calls.analysis_entry(dict(ctx, **a, **b)) for a in ({}, dict(N0=1))
           for b in ({}, dict(psig=1), dict(sp6=1), dict(sp6=1, psig=1))} | {_calls.analysis_entry(dict(ctx, satrep=1))}
    bat = dict(q14=1)
    got |= {_calls.analysis_entry(dict(bat, **a, **b)) for a in ({}, dict(N0=1)) for b in ({}, dict(sp6=1))}
    got |= {_calls.analysis_entry(dict(bat, satrep=1)), _calls.analysis_entry(dict(bat, nsigma=3, which=None))}
    got |= {_calls.analysis_entry(dict(bat, nsigma=3, which=1, **a, **b)) for a in ({}, dict(N0=1)) for b in ({}, dict(sp6=1))}
    assert got == {n for n in _calls.TABLE if "track_mc" not in n}
