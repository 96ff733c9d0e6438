"""The host-side staging of the _host forms of the sampled calls and of the order statistics under AddressSanitizer and
UndefinedBehaviorSanitizer, without a GPU: tests/host_staging_asan.cpp (a stand-alone program with its own main and its own small HIP
runtime in which device memory is malloc'd host memory of exactly the size asked for, and a launch does nothing) linked with the three
translation units compiled for the host only.  A staging buffer that is too small, a copy that is too long, a leak or a use after free
ends the program with a sanitizer report.  Nothing here is loaded into python."""
import os
import subprocess

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "successiveconvexification_amd", "csrc")
UNITS = ("scvx_mc.hip", "scvx_mc_nav.hip", "scvx_quantile.hip")


def _clangxx():
    """the clang++ behind hipcc (hipcc itself adds its GPU runtime to a link)"""
    root = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    for cand in (os.path.join(root, "llvm", "bin", "clang++"), os.path.join(root, "lib", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    raise AssertionError("no clang++ next to %s" % HIPCC)


def test_host_staging_is_clean_under_asan_and_ubsan(tmp_path):
    # host code only: every sanitizer option goes to the host compilation (-Xarch_host), nothing is built for the GPU
    san = ["-Xarch_host", "-fsanitize=address,undefined"]
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g"] + san + ["-Xarch_host", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    jobs = []
    for src in [os.path.join(CSRC, f) for f in UNITS] + [os.path.join(ROOT, "tests", "host_staging_asan.cpp")]:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        jobs.append((obj, subprocess.Popen([HIPCC] + flags + ["-x", "hip", "-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for obj, pr in jobs:
        out = pr.communicate()[0].decode()
        assert pr.returncode == 0, out
    exe = str(tmp_path / "host_staging_asan")
    # the fat binary the host objects refer to does not exist in a host-only build: the program's runtime never reads it
    link = subprocess.run([_clangxx()] + san + ["-Wl,--unresolved-symbols=ignore-in-object-files", "-o", exe] + [o for o, _ in jobs],
                          capture_output=True, text=True)
    assert link.returncode == 0, link.stdout + link.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sanitizers on" in run.stdout                              # the objects really are instrumented
    assert "host staging:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
