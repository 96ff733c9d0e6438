"""The aerodynamic body torque (SCVX_MODEL_AERO_TORQUE, include/scvx.h) without a GPU: the independent torch reference
(tests/aero_torque_reference.py) pinned to the frozen oracle with the torque off and to the host mirror's numeric torque, the flag through
header / bindings / sample problems / Julia shim, the torque fixtures reproduced, and the torque kernels' metadata in the built library."""
import os
import re
import subprocess
from dataclasses import replace

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, random_segments

AERO_TRQ = os.path.join(GOLDEN, "oracle_scvx_aero_torque_batch4_tol1e-08.npz")
AEROFIN_TRQ = os.path.join(GOLDEN, "oracle_scvx_aerofin_torque_tol1e-08.npz")


def _oracle_problem(kind, aero_tables):
    from oracle import model
    aero = model.AeroData(*aero_tables)
    return {"exo": model.base_prob_scaled(), "aero": model.base_prob_scaled(aero),
            "exo+fins": model.base_prob_fin_scaled(), "aero+fins": model.base_prob_fin_scaled(aero)}[kind]


def _segments(po, B, K, seed):
    x, u, sigma = random_segments(po, B, K, seed)
    if po.fins:
        u = np.concatenate([u, po.finmxf * np.random.default_rng(seed + 1).uniform(-0.7, 0.7, (B, K + 1, 2))], axis=-1)
    return x, u, sigma


@pytest.mark.parametrize("npts", [1, 3, 10])
@pytest.mark.parametrize("kind", ["exo", "aero", "exo+fins", "aero+fins"])
def test_reference_without_torque_matches_the_oracle(kind, npts, aero_tables):
    """Spline, clamp, first-order hold and RK4 of the torch reference are the oracle's: with the torque off the two agree to rounding,
    so the torque is the only thing the reference adds."""
    import aero_torque_reference as ref
    from oracle import dynamics as od
    po = _oracle_problem(kind, aero_tables)
    B, K = 3, 9
    x, u, sigma = _segments(po, B, K, 20261010 + npts)
    dt = 1.0 / (K + 1)
    e_ref, d_ref = od.linearize(od.Params(po), x, u, sigma, dt, npts)
    par = ref.Params(po)
    e, d = ref.linearize(par, x, u, sigma, dt, npts)
    scale = max(1.0, np.abs(d_ref).max())
    assert np.abs(e - e_ref).max() < 1e-12
    assert np.abs(d - d_ref).max() < 1e-11 * scale, (np.abs(d - d_ref).max(), scale)
    assert np.abs(ref.propagate(par, x, u, sigma, dt, npts) - e_ref).max() < 1e-12
    if po.aero is not None:   # and the torque does change the rate rows
        _, dt_ = ref.linearize(ref.Params(po, torque=True), x, u, sigma, dt, npts)
        assert np.abs(dt_ - d)[..., 11:14].max() > 1e-6


def _torque_at(q, v, aero_tables):
    import aero_torque_reference as ref
    import torch
    from oracle import model
    par = ref.Params(model.base_prob_scaled(model.AeroData(*aero_tables)), torque=True)
    _, tau = ref.aero_terms(par, torch.tensor(q, dtype=torch.float64), torch.tensor(v, dtype=torch.float64))
    return tau.numpy(), par


def test_torque_term_equals_the_host_mirror_times_the_unnormalised_length(aero_tables):
    """tau = T (v x bv) (the symbolic aero_force, ifnz: un-normalised) against the host mirror aerodynamics.aero_force, the NUMERIC
    method (normalised direction): two separately written codes, tau = mirror_torque * |v x bv| wherever the mirror has a torque."""
    from successiveconvexification_amd import aerodynamics, sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData
    pp = sp.base_prob_aero_scaled(AtmosphericData(*aero_tables), torque=True)
    rng = np.random.default_rng(20261011)
    n = 0
    for _ in range(60):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        v = rng.normal(size=3)
        v *= rng.uniform(0.05, 1.4) * pp.sos / np.linalg.norm(v)    # Mach 0.05 .. 1.4: inside the table
        tau, par = _torque_at(q, v, aero_tables)
        bv = np.array([1 - 2 * (q[2] ** 2 + q[3] ** 2), 2 * (q[1] * q[2] + q[0] * q[3]), 2 * (q[1] * q[3] - q[0] * q[2])])
        if abs(bv @ v) / np.linalg.norm(v) >= 0.95:
            continue                                                  # the numeric method's drag-only branch
        _, trq = aerodynamics.aero_force(pp.aero, bv, v, pp.sos)
        want = trq * np.linalg.norm(np.cross(v, bv))
        assert np.abs(tau - want).max() < 1e-13 * np.abs(want).max(), (tau, want)
        n += 1
    assert n >= 40


def test_torque_term_vanishes_along_the_body_axis_and_at_rest(aero_tables):
    q = np.array([0.9, 0.1, -0.3, 0.2])
    q /= np.linalg.norm(q)
    bv = np.array([1 - 2 * (q[2] ** 2 + q[3] ** 2), 2 * (q[1] * q[2] + q[0] * q[3]), 2 * (q[1] * q[3] - q[0] * q[2])])
    for v in (0.7 * bv, -1.3 * bv):     # v x bv is zero up to the rounding of the cross product of two parallel vectors
        tau, _ = _torque_at(q, v, aero_tables)
        assert np.abs(tau).max() < 1e-30, (v, tau)
    tau, _ = _torque_at(q, np.zeros(3), aero_tables)
    assert np.all(tau == 0.0), tau


def test_flag_in_header_bindings_sample_problems_and_julia(aero_tables):
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData, DescentProblem
    h = open(os.path.join(ROOT, "include", "scvx.h")).read()
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SCVX_MODEL_(\w+) (\d+)", h)}
    assert bits == {"DPMAX": 1, "FINS": 2, "AERO_TORQUE": 4}
    assert DescentProblem(model_flags=4).aero_torque and not DescentProblem(model_flags=3).aero_torque
    a = AtmosphericData(*aero_tables)
    pa = sp.base_prob_aero_scaled(a, torque=True)
    assert pa.model_flags == 4 and pa.aero_torque and pa.nu == 3 and pa.to_c().model_flags == 4 and pa.to_c().aero_kind == 1
    assert sp.base_prob_aero_scaled(a).model_flags == 0                 # the default is today's model
    pf = sp.base_prob_fin_scaled(a, torque=True)
    assert pf.model_flags == 6 and pf.aero_torque and pf.fins and pf.nu == 5
    assert sp.base_prob_fin_scaled(a).model_flags == 2
    with pytest.raises(ValueError):
        sp.base_prob_fin_scaled(None, torque=True)                      # no torque without aerodynamic data
    # the torque-on problem differs from the torque-off one in the flag only
    p0 = sp.base_prob_aero_scaled(a)
    assert replace(pa, model_flags=0).to_c().jB[:] == p0.to_c().jB[:] and pa.aero.length_scalar == p0.aero.length_scalar
    jl = open(os.path.join(ROOT, "julia", "ScvxAMD.jl")).read()
    assert re.search(r"^const MODEL_AERO_TORQUE = 4\b", jl, re.M)
    assert re.search(r"model_flags=\$\(@__MODULE__\)\.MODEL_FLAGS\[\]", jl)


def _load(path):
    assert os.path.exists(path), path
    return np.load(path)


def test_torque_fixtures_are_what_their_script_says(aero_tables):
    """The fixtures of tests/golden/make_oracle_torque_runs.py: layout, initial conditions, and the first two steps of one trajectory of
    each re-run through the oracle's loop on the torque discretisation."""
    import importlib.util
    from oracle import model
    spec = importlib.util.spec_from_file_location("make_oracle_torque_runs", os.path.join(GOLDEN, "make_oracle_torque_runs.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = _load(AERO_TRQ)
    p = gen.problem(False)
    assert list(g["index"]) == [0, 68, 161, 255] and float(g["tol"]) == 1e-8 and int(g["seed"]) == 20261003 and int(g["B"]) == 256
    assert np.array_equal(model.disperse_ics(p, 256, 20261003)[g["index"]], g["ic"])
    assert g["log"].shape == (4, p.imax - 1, 7) and g["xs"].shape == (4, p.imax - 1, p.K + 1, 14) and g["us"].shape == (4, p.imax - 1, p.K + 1, 3)
    f = _load(AEROFIN_TRQ)
    pf = gen.problem(True)
    assert f["xs"].shape == (1, pf.imax - 1, 51, 14) and f["us"].shape == (1, pf.imax - 1, 51, 5)
    assert np.array_equal(f["ic"][0], np.concatenate([pf.rIi, pf.vIi]))
    for gg, pp, j in ((g, p, 2), (f, pf, 0)):
        log, xs, us = gen.run_steps(pp, gg["ic"][j], 2)
        assert np.array_equal(log[:, 3], gg["log"][j, :2, 3])
        assert np.allclose(log[:, 1:6], gg["log"][j, :2, 1:6], rtol=1e-9, atol=1e-9, equal_nan=True)   # |delta| = Inf on a first step
        assert np.abs(xs - gg["xs"][j, :2]).max() < 1e-9 and np.abs(us - gg["us"][j, :2]).max() < 1e-9


# private segment (bytes per lane) of the torque instantiations measured when they were written (hipcc, gfx950); the torque-free
# counterparts are unchanged (aero / aero+fins split producer, fp64: 332 / 460)
TRQ_PRIVATE_MAX = {"double": 476, "float": 1964}


def test_torque_kernels_exist_with_bounded_private_memory(tmp_path):
    """Kernel metadata of the built library (no GPU): the four kernel forms (split producer, persistent / one-group producer-consumer,
    propagate) are instantiated with the torque for fp64, fp64 with float tiles and fp32, models aero and aero + fins: 22 kernels."""
    import shutil
    from successiveconvexification_amd import build
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    lib = tmp_path / "lib.so"
    shutil.copy(build.build(), lib)
    subprocess.run([objdump, "--offloading", str(lib)], cwd=tmp_path, check=True, capture_output=True)
    kernels = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        cur = {}
        for line in notes.splitlines():
            m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
            if not m:
                continue
            k, v = m.groups()
            if k == "args" or (k == "agpr_count" and cur.get("name")):
                if cur.get("name"):
                    kernels[cur["name"]] = cur
                cur = {}
            cur[k] = v
        if cur.get("name"):
            kernels[cur["name"]] = cur
    # the torque is the last template argument of the four kernel forms: ...ILb1E...Lb1EEEv (true, end of arguments, end of name)
    trq = {n: k for n, k in kernels.items() if re.search(r"(linearize_pc|linearize_pcp|linearize_pcp2|propagate)_kernelI.*Lb1EEEv", n)}
    forms = {f: sum(1 for n in trq if f in n) for f in ("linearize_pcp2_kernel", "linearize_pcp_kernel", "linearize_pc_kernel", "propagate_kernel")}
    assert forms == {"linearize_pcp2_kernel": 6, "linearize_pcp_kernel": 6, "linearize_pc_kernel": 6, "propagate_kernel": 4}, forms
    assert not any("linearize_kernel" in n for n in trq)      # the column-per-lane form has no torque instantiation
    for n, k in trq.items():
        prec = {"d": "double", "f": "float"}[re.search(r"_kernelI(?:Lb[01]E)+([df])", n).group(1)]   # the arithmetic type R
        assert int(k["private_segment_fixed_size"]) <= TRQ_PRIVATE_MAX[prec], (n, k["private_segment_fixed_size"])
