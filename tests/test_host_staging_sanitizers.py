"""The host-side staging of the _host forms (the sampled calls, the order statistics, the covariance and navigation analyses, plan
tracking) under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU: tests/host_staging_asan.cpp (a stand-alone program with
its own main and its own small HIP runtime in which device memory is malloc'd host memory of exactly the size asked for, and a launch
does nothing) linked with the translation units compiled for the host only.  A staging buffer that is too small, a copy that is too
long, a leak or a use after free ends the program with a sanitizer report.  The program's runtime also counts what every call allocates,
copies, launches and synchronises -- tests/golden/host_staging_traffic.txt holds those counts as the hand-written staging sequences made
them, before csrc/scvx_stage.hpp replaced them -- and makes every allocation, copy and launch of one call of each form fail in turn.
Nothing here is loaded into python."""
import os
import subprocess

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "successiveconvexification_amd", "csrc")
UNITS = ("scvx_mc.hip", "scvx_mc_nav.hip", "scvx_quantile.hip", "scvx_cov.hip", "scvx_nav.hip", "scvx_track.hip")
# the _host forms whose error path the program sweeps
SWEPT = ("scvx_track_gains_f64_host", "scvx_track_fly_f64_host", "scvx_track_fly_nav_f64_host", "scvx_cov_propagate_f64_host",
         "scvx_cov_path_sigma_f64_host", "scvx_nav_cov_f64_host", "scvx_nav_path_sigma_f64_host", "scvx_mc_draws_f64_host",
         "scvx_track_mc_q_f64_host", "scvx_track_mc_nav_q_f64_host", "scvx_order_stats_f64_host")


def _clangxx():
    """the clang++ behind hipcc (hipcc itself adds its GPU runtime to a link)"""
    root = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    for cand in (os.path.join(root, "llvm", "bin", "clang++"), os.path.join(root, "lib", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    raise AssertionError("no clang++ next to %s" % HIPCC)


def build_program(tmp_path, csrc=CSRC):
    """the program linked with the translation units of `csrc`, every one instrumented; returns its path"""
    # host code only: every sanitizer option goes to the host compilation (-Xarch_host), nothing is built for the GPU
    san = ["-Xarch_host", "-fsanitize=address,undefined"]
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g"] + san + ["-Xarch_host", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", csrc]
    jobs = []
    for src in [os.path.join(csrc, f) for f in UNITS] + [os.path.join(ROOT, "tests", "host_staging_asan.cpp")]:
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
    return exe


def golden_lines(name, prefix, keep=lambda line: True):
    """the lines of tests/golden/<name>, every one beginning with `prefix`, that `keep` selects"""
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        want = f.read().splitlines()
    assert all(line.startswith(prefix) for line in want)
    return [line for line in want if keep(line)]


def require_same_lines(got, want, at_least):
    assert len(want) > at_least
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_host_staging_is_clean_under_asan_and_ubsan(tmp_path):
    exe = build_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(run.stdout[-4000:], run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr
    assert "sanitizers on" in run.stdout                              # the objects really are instrumented
    assert "host staging:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
    # the same allocations, copies, launches and synchronises, call by call, as the staging code made before the helper: equality
    require_same_lines([line for line in run.stdout.splitlines() if line.startswith("traffic ")],
                       golden_lines("host_staging_traffic.txt", "traffic "), 200)
    # what the sampled calls refuse, in which words, and which of two faults wins: as the six hand-written bodies had it
    require_same_lines([line for line in run.stdout.splitlines() if line.startswith("refusal ")],
                       golden_lines("mc_refusals.txt", "refusal ", lambda line: "_veh_" not in line), 700)
    # the same for the covariance and navigation analyses (their _vehicle forms: tests/test_host_staging_cov_vehicle_sanitizers.py)
    require_same_lines([line for line in run.stdout.splitlines() if line.startswith("cov-refusal ")],
                       golden_lines("cov_refusals.txt", "cov-refusal ", lambda line: "_vehicle_" not in line), 300)
    # every allocation, copy and launch of one call of each form was made to fail, and the error contract held
    swept = [line.split()[2].rstrip(":") for line in run.stdout.splitlines() if line.startswith("error path ")]
    assert swept == list(SWEPT)
