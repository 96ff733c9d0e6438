"""The executor primitives of the conic kernel (K4) in isolation (tools/micro/k4_executor_ab.hip): WaveExT<3>, WaveExT<5>, BlockEx<2, .> and
BlockEx<4, .> against long-double arithmetic on the host -- tile_gemm and the accumulator products (every tail of the 4-wide k-slots, nb
1 / 4 / 14, row-major / transposed / padded strides, alpha 1 / -1 / 0.37, acc and add both ways, a sentinel around the 14 x nb block), sum /
min / all with one lane different from the rest at every lane position, and the block recurrences chain / chain_n / chain_range_n forward
and reverse at K = 1, 2, 3, 9, 50.  The localiser of tests/test_gpu_k4_path.py: when the path test fails, this says which brick is wrong.

Bounds are derived, not measured (u = 2^-53): a product of depth n within (n + 2) u sum |a_k| |b_k| (any order of summation, with or
without FMA), the chains by the same bound carried along the recursion, sum within (lanes) u sum |x|, min and all exact.  The program
prints the worst ratio of error to bound per executor and primitive and exits non-zero above 1."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXECUTORS = ("WaveExT<3>", "WaveExT<5>", "BlockEx<2,3>", "BlockEx<2,5>", "BlockEx<4,3>", "BlockEx<4,5>")
PRIMITIVES = ("tile_gemm", "acc_mac_store", "acc_mac_twice", "acc_store_init", "sum", "min", "all", "chain", "chain_n1", "chain_n2", "chain_n4",
              "chain_range_n")


def test_executor_primitives_against_long_double(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    exe = tmp_path / "k4_executor_ab"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "successiveconvexification_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "micro", "k4_executor_ab.hip")], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for m in re.finditer(r"^(\S+)\s+(\S+)\s+worst error / bound (\S+)\s+\((\d+) values, (\d+) outside", r.stdout, flags=re.M):
        seen[(m.group(1), m.group(2))] = (float(m.group(3)), int(m.group(4)), int(m.group(5)))
    for ex in EXECUTORS:
        for p in PRIMITIVES:
            assert (ex, p) in seen, (ex, p)
            ratio, n, bad = seen[(ex, p)]
            assert ratio <= 1.0 and n > 0 and bad == 0, (ex, p, ratio, n, bad)
