"""The host-side staging of the vehicle errors in the first-order analyses under AddressSanitizer and UndefinedBehaviorSanitizer,
without a GPU: tests/host_staging_cov_vehicle_asan.cpp (a stand-alone program with its own main; the HIP runtime, in which device memory
is malloc'd host memory of exactly the size asked for and a launch does nothing, is that of tests/host_staging_asan.cpp) linked with
the translation units compiled for the host only -- the recipe of tests/test_host_staging_sanitizers.py with the vehicle tiles' unit
added.  The program itself requires that the _vehicle forms without vtile, sens and dense outputs stage what the path-sigma calls
stage, that each optional array costs one copy of its documented size, that a refusal allocates nothing and that every allocation,
copy and launch made to fail leaves nothing behind.  Nothing here is loaded into python."""
import os
import subprocess

import test_host_staging_sanitizers as hs
from conftest import ROOT

UNITS = hs.UNITS + ("scvx_vtile.hip",)
SWEPT = ("scvx_vehicle_tiles_f64_host", "scvx_cov_vehicle_f64_host", "scvx_nav_cov_vehicle_f64_host")


def build_program(tmp_path):
    """hs.build_program's flags and link, for this program and its units; returns the program's path"""
    san = ["-Xarch_host", "-fsanitize=address,undefined"]
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g"] + san + ["-Xarch_host", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", hs.CSRC, "-I", os.path.join(ROOT, "tests")]
    jobs = []
    for src in [os.path.join(hs.CSRC, f) for f in UNITS] + [os.path.join(ROOT, "tests", "host_staging_cov_vehicle_asan.cpp")]:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        jobs.append((obj, subprocess.Popen([hs.HIPCC] + flags + ["-x", "hip", "-c", src, "-o", obj], stdout=subprocess.PIPE,
                                           stderr=subprocess.STDOUT)))
    for obj, pr in jobs:
        out = pr.communicate()[0].decode()
        assert pr.returncode == 0, out
    exe = str(tmp_path / "host_staging_cov_vehicle_asan")
    link = subprocess.run([hs._clangxx()] + san + ["-Wl,--unresolved-symbols=ignore-in-object-files", "-o", exe] + [o for o, _ in jobs],
                          capture_output=True, text=True)
    assert link.returncode == 0, link.stdout + link.stderr
    return exe


def test_cov_vehicle_staging_is_clean_under_asan_and_ubsan(tmp_path):
    exe = build_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(run.stdout[-3000:], run.stderr)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr
    assert "sanitizers on" in run.stdout                              # the objects really are instrumented
    assert "host staging (vehicle errors, first-order analyses):" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
    calls = [line for line in run.stdout.splitlines() if line.startswith("traffic covveh ") and "_vehicle_" in line]
    assert len(calls) == 5 * 8                                        # five scenarios: one tile call, four covariance and three navigation forms
    swept = [line.split()[2].rstrip(":") for line in run.stdout.splitlines() if line.startswith("error path ")]
    assert swept == list(SWEPT)
    # what the _vehicle forms refuse, in which words, and which of two faults wins: as the hand-written bodies had it
    hs.require_same_lines([line for line in run.stdout.splitlines() if line.startswith("cov-refusal ")],
                          hs.golden_lines("cov_refusals.txt", "cov-refusal ", lambda line: "_vehicle_" in line), 150)
