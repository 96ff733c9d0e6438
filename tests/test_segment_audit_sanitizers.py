"""The host-side staging of scvx_segment_audit_f64_host under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU:
tests/segment_audit_asan.cpp (a stand-alone program with its own main and its own small HIP runtime, as tests/host_staging_asan.cpp)
linked with csrc/scvx_audit.hip compiled for the host only.  A staging buffer that is too small, a copy that is too long, a leak or a
use after free ends the program with a sanitizer report; every allocation, copy and launch of a call is made to fail in turn.  Nothing
here is loaded into python."""
import os
import subprocess

from conftest import ROOT
from test_host_staging_sanitizers import CSRC, HIPCC, _clangxx


def test_segment_audit_staging_is_clean_under_asan_and_ubsan(tmp_path):
    # host code only: every sanitizer option goes to the host compilation (-Xarch_host), nothing is built for the GPU
    san = ["-Xarch_host", "-fsanitize=address,undefined"]
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g"] + san + ["-Xarch_host", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    jobs = []
    for src in (os.path.join(CSRC, "scvx_audit.hip"), os.path.join(ROOT, "tests", "segment_audit_asan.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        jobs.append((obj, subprocess.Popen([HIPCC] + flags + ["-x", "hip", "-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for obj, pr in jobs:
        out = pr.communicate()[0].decode()
        assert pr.returncode == 0, out
    exe = str(tmp_path / "segment_audit_asan")
    # the fat binary the host objects refer to does not exist in a host-only build: the program's runtime never reads it
    link = subprocess.run([_clangxx()] + san + ["-Wl,--unresolved-symbols=ignore-in-object-files", "-o", exe] + [o for o, _ in jobs],
                          capture_output=True, text=True)
    assert link.returncode == 0, link.stdout + link.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(run.stdout[-4000:], run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr
    assert "sanitizers on" in run.stdout                              # the objects really are instrumented
    assert "segment audit staging: clean" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
    traffic = [line for line in run.stdout.splitlines() if line.startswith("traffic ")]
    assert len(traffic) == 16
    # exactly the five arrays of the call, of exactly their sizes, each freed: B = 65, K = 3, NU = 3 with the report
    n = 8 * (65 * 4 * 17 + 65 + 65 * 3 * 11 + 65 * 16)
    assert "traffic NU 3 B 65 K 3 report 1: allocs 5 (%d B) frees 5 h2d 3 (%d B) d2h 2 (%d B) launches 2 syncs 1" % (
        n, 8 * (65 * 4 * 17 + 65), 8 * (65 * 3 * 11 + 65 * 16)) in traffic
