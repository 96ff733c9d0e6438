"""The C traffic of the Python binding of the analysis and dispersion calls, pinned without a shared library or a device.

tests/golden/py_call_traffic.txt holds, for every call dynamics.py and batch.py make over the stand-in library of
tests/py_call_recorder.py, the entry point, every scalar, every struct's bytes, every array's dtype and shape and the checksum of every
input array -- and every ValueError of these functions, singly and in pairs.  tests/golden/make_py_call_traffic.py wrote it and
regenerates the lines here; they must agree byte for byte, so an argument in the wrong position, a changed refusal or a changed order of
refusals shows up on the CPU."""
import importlib.util
import os
import re

from conftest import GOLDEN

FAMILIES = r"scvx_(cov|nav|track_mc|batch_(cov|nav_cov|track_mc|margins_from|thrust_margins_from))\w*"


def _maker():
    spec = importlib.util.spec_from_file_location("make_py_call_traffic", os.path.join(GOLDEN, "make_py_call_traffic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_binding_makes_the_recorded_calls_and_refusals():
    want = open(os.path.join(GOLDEN, "py_call_traffic.txt")).read().split("\n")
    assert want[-1] == ""
    got = _maker().traffic_lines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d:\n  now      %s\n  recorded %s" % (i + 1, a, b)
    assert len(got) == len(want) - 1


def test_the_recording_covers_every_entry_point_of_the_two_families():
    """every _host and scvx_batch_ form of the two families that include/scvx.h declares is called at NU = 3 and at NU = 5, and no refusal
    case went through to the library unnoticed"""
    from py_call_recorder import header_params
    names = sorted(n for n in header_params() if re.fullmatch(FAMILIES, n) and (n.endswith("_host") or n.startswith("scvx_batch_")))
    assert len(names) == 33, names
    text = open(os.path.join(GOLDEN, "py_call_traffic.txt")).read()
    parts = re.split(r"^# NU = (\d), \w[\w-]*: \d+ calls$", text.split("# refusals")[0], flags=re.M)
    called = {3: set(), 5: set()}
    for nu, body in zip(parts[1::2], parts[2::2]):
        called[int(nu)] |= set(re.findall(r"^(scvx_\w+)\(", body, flags=re.M))
    for nu in (3, 5):
        assert set(names) <= called[nu], (nu, set(names) - called[nu])
    refusals, pairs = re.findall(r"^refusal .*$", text, flags=re.M), re.findall(r"^pairs .*$", text, flags=re.M)
    decided = sum(len(re.findall(r" [><=!][a-z_0-9]+", re.sub(r"\{[^}]*\}", "", p.split("]", 1)[1]))) for p in pairs)
    assert len(refusals) > 300 and decided > 2500, (len(refusals), decided)
    assert "no refusal" not in "".join(refusals + pairs)
