"""K1's persistent group walk and skip list on the MI355X, element by element against the oracle.

From three substeps up K1 runs as persistent blocks (linearize_pcp_kernel, linearize_pcp2_kernel), one per CU; block b walks the
groups b, b + grid, ...  What is particular to these kernels sits in that walk: every role fetches the inputs of its NEXT group before
the stores of the current one are issued, the tile stores of group g drain while group g + 1 integrates, the stage ring and the tile
region are reused group after group, advance() jumps over groups the skip list marks unchanged, the last group is ragged, and with
NB = 2 a consumer lane carries two segment batches of which the second may lie wholly past the end.  The other parity files stop at
1,920 segments: a block there runs one group.  Here the batch comes from tests/k1_walk_reference.py (walk_shape): at the largest group
(36 segments) some blocks walk three groups and the rest two, every other form walks more, and every form ends on a ragged group --
about 20,700 segments at 256 CUs.  Bounds are the project's per-segment ones and do not depend on the batch: endpoint 1e-12, derivative
1e-11 * max(1, |d_ref|max), |K2 - K1 endpoint| < 1e-13; the float forms 2e-5 / 2e-4 relative as tests/test_gpu_discretize.py states them.

A failure names the worst segment with its group, round, block and place in the group for the form's NS, so the message says where in
the walk it went wrong (k1_walk_reference.describe).

Not reached: linearize_pcp_kernel<true, R, O> without fins or torque (the aero branch of the `else if (persist)` arm of
launch_linearize_t).  `split` is false for the aero model only with SCVX_K1_SG=0, and then `persist` (which asks for sg, fins or torque)
is false as well, so no setting of the default build launches it.
"""
import time
from dataclasses import replace

import numpy as np
import pytest

import k1_walk_reference as w
from conftest import random_segments

pytestmark = pytest.mark.gpu

K13 = 13
_REF = {}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _problems(model_name, aero_tables, K=None):
    """(product problem, oracle problem, torque) of "exo" | "aero" | "fins" | "aero+fins" | "aero+torque" | "aero+fins+torque" """
    from oracle import model
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData
    parts = model_name.split("+")
    aero, fins, torque = "aero" in parts, "fins" in parts, "torque" in parts
    a = AtmosphericData(*aero_tables) if aero else None
    oa = model.AeroData(*aero_tables) if aero else None
    if fins:
        pp, po = sp.base_prob_fin_scaled(a, torque=torque), model.base_prob_fin_scaled(oa)
    elif aero:
        pp, po = sp.base_prob_aero_scaled(a, torque=torque), model.base_prob_scaled(oa)
    else:
        pp, po = sp.base_prob_scaled, model.base_prob_scaled()
    if K is not None:
        pp, po = replace(pp, K=K), replace(po, K=K)
    return pp, po, torque


def _segments(po, B, K, seed):
    """random_segments plus the fin columns as test_gpu_fins._fin_segments makes them; every trajectory has its own sigma"""
    x, u, sigma = random_segments(po, B, K, seed)
    if getattr(po, "fins", False):
        fin = po.finmxf * np.random.default_rng(seed + 1).uniform(-0.7, 0.7, (B, K + 1, 2))
        u = np.concatenate([u, fin], axis=-1)
    return x, u, sigma


def _oracle(po, torque, x, u, sigma, dt, npts):
    if torque:
        import aero_torque_reference as ref
        return ref.linearize(ref.Params(po, torque=True), x, u, sigma, dt, npts)
    from oracle import dynamics as od
    return od.linearize(od.Params(po), x, u, sigma, dt, npts)


def _special_nodes(x, K, cus):
    """the two special nodes of test_linearize_matches_oracle_aero, v = 0 (ifnz guards) and v along the body axis (no lift), in segments
    that the 36-segment walk reaches in the SECOND round of block 5 and in the LAST (third) round of block 3.

    This case found the pipeline kernels 4.447e-10 off (bound 9.69e-11) in the segment of the second node, in any round and alone as
    well, going as 1 / npts: with v exactly along the body axis c v - |v|^2 bv left a fused-multiply-add residue of 1e-18 as lift
    direction where the model has none, and 1 / ln made a derivative of 1e-7 of it in the first stage.  scvx_dyn.hpp lift_dir_defined
    now takes a length within 64 ulps of the cancelling terms as no direction; 5.3e-15 since (profiles/k1_walk_parity.md)."""
    nseg = x.shape[0] * K
    grid = w.grid_of(nseg, 36, cus)
    seg_a, seg_b = (grid + 5) * 36 + 17, (2 * grid + 3) * 36 + 20
    assert w.locate(seg_a, 36, grid)[:2] == (grid + 5, 1) and w.locate(seg_b, 36, grid)[:2] == (2 * grid + 3, 2)
    assert seg_b < nseg and 3 * grid + 3 >= w.ngrp_of(nseg, 36)          # round 2 is block 3's last
    x[seg_a // K, seg_a % K, 4:7] = 0.0
    x[seg_b // K, seg_b % K, 7:11] = [1, 0, 0, 0]
    x[seg_b // K, seg_b % K, 4:7] = [-0.2, 0, 0]


def _reference(model_name, B, K, npts, aero_tables, special=False):
    """segments and the reference's K1 result, once per (model, shape, npts): shared by the kernel forms, and never written to"""
    key = (model_name, B, K, npts, special)
    if key not in _REF:
        po, torque = _problems(model_name, aero_tables)[1:]
        x, u, sigma = _segments(po, B, K, 20261018 + B)
        if special:
            _special_nodes(x, K, _cus())
        e_ref, d_ref = _oracle(po, torque, x, u, sigma, 1.0 / (K + 1), npts)
        for a in (x, u, sigma, e_ref, d_ref):
            a.setflags(write=False)
        _REF[key] = (x, u, sigma, e_ref, d_ref)
    return _REF[key]


def _walk(form, nseg, cus, rounds):
    """(ns, grid) of a form, and that the launch is the one this file is about: more than `rounds` groups per block somewhere, ragged end"""
    f = w.FORMS[form]
    ns = f["ns"]
    grid = w.grid_of(nseg, ns, cus, f["persistent"])
    if f["persistent"]:
        assert grid == cus and w.ngrp_of(nseg, ns) >= rounds * cus + cus // 4, (form, nseg, cus)
    assert nseg % ns != 0
    return ns, grid


# id, model, npts, K, environment, form (tests/k1_walk_reference.FORMS), kernel instantiation and the part of the walk it is there for
DIRECT = [
    ("exo", "exo", 4, 13, {}, "exo pcp",
     "linearize_pcp_kernel<false, double, double, false, 1>: 28-segment groups, 3 rounds; closed-form r / v columns written per group"),
    ("aero", "aero", 4, 13, {}, "aero split pcp2",
     "linearize_pcp2_kernel<true, double, double, false>: NB = 2, 36-segment groups; blocks with 3 and with 2 groups; the ragged group's second batch lies past nseg"),
    ("fins", "fins", 3, 13, {}, "fins exo split pcp2",
     "linearize_pcp2_kernel<false, double, double, true>: NB = 1, 12-segment groups, 7 rounds: the longest walk"),
    ("aero+fins", "aero+fins", 3, 13, {}, "fins + aero split pcp2",
     "linearize_pcp2_kernel<true, double, double, true>: NB = 2, 24-segment groups, 4 rounds"),
    ("aero+torque", "aero+torque", 3, 13, {}, "aero split pcp2",
     "linearize_pcp2_kernel<true, double, double, false, true>: the wider torque record in ring and hand-over slots reused per group"),
    ("aero+fins+torque", "aero+fins+torque", 3, 13, {}, "fins + aero split pcp2",
     "linearize_pcp2_kernel<true, double, double, true, true>"),
    ("aero+fins,SG=0", "aero+fins", 3, 13, {"SCVX_K1_SG": "0"}, "fins (+ torque) pcp (SG=0)",
     "linearize_pcp_kernel<true, double, double, true>: the non-split persistent kernel with FIN, 14-segment groups, 6 rounds"),
    ("aero+torque,SG=0", "aero+torque", 3, 13, {"SCVX_K1_SG": "0"}, "aero + torque pcp (SG=0)",
     "linearize_pcp_kernel<true, double, double, false, 1, true>: the non-split persistent kernel with TRQ, 21-segment groups"),
    ("exo,PERSIST=1,npts=1", "exo", 1, 13, {"SCVX_K1_PERSIST": "1"}, "exo pcp",
     "linearize_pcp_kernel<false, ...> with a single substep: the prefetch and the stores of a group are four stages apart"),
    ("exo,K=1", "exo", 4, 1, {}, "exo pcp",
     "every segment its own trajectory: fetch() and sigma_of() index a new trajectory per lane, same segment count"),
    ("exo,K=100", "exo", 4, 100, {}, "exo pcp",
     "a group inside one trajectory; three to four groups per trajectory"),
    ("aero,special nodes", "aero", 4, 13, {}, "aero split pcp2",
     "v = 0 and v along the body axis in segments of a block's second and last round: the guarded branches on prefetched inputs"),
]


@pytest.mark.parametrize("name,model_name,npts,K,env,form,what", DIRECT, ids=[c[0] for c in DIRECT])
def test_direct_entry_walk_matches_the_oracle(name, model_name, npts, K, env, form, what, aero_tables, monkeypatch):
    """(a) linearize_batch / propagate_batch in every persistent form that the default build can launch (DIRECT: instantiation and
    reason per case) against oracle.dynamics.linearize, with the torque against tests/aero_torque_reference.py.  The two torque models
    use the shape with ngrp(36) >= cus + cus / 4 (blocks with two groups and with one at NS = 36; two and three rounds at 24 and 21):
    their automatic-differentiation reference costs seconds per ten thousand segments."""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch, propagate_batch
    cus = _cus()
    torque = "torque" in model_name
    rounds = 1 if torque else 2
    B = w.walk_shape(cus, K13, rounds) * K13 if K == 1 else w.walk_shape(cus, K, rounds)
    ns, grid = _walk(form, B * K, cus, rounds)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t0 = time.perf_counter()
    x, u, sigma, e_ref, d_ref = _reference(model_name, B, K, npts, aero_tables, special="special" in name)
    t1 = time.perf_counter()
    pp = _problems(model_name, aero_tables)[0]
    dt = 1.0 / (K + 1)
    c = IntegratorCache(pp, npts=npts)
    e, d = linearize_batch(c, x, u, sigma, dt)
    xn = propagate_batch(c, x, u, sigma, dt)
    c.close()
    t2 = time.perf_counter()
    scale = max(1.0, np.abs(d_ref).max())
    print("K1 walk %-22s B %5d K %3d npts %d  NS %2d grid %3d groups %4d: endpoint %.2e  derivative %.2e (scale %.2f)  K2 %.2e  K2-K1 %.2e"
          "  [reference %.2f s, device %.2f s]"
          % (name, B, K, npts, ns, grid, w.ngrp_of(B * K, ns), np.abs(e - e_ref).max(), np.abs(d - d_ref).max(), scale,
             np.abs(xn - e_ref).max(), np.abs(xn - e).max(), t1 - t0, t2 - t1))
    assert np.isfinite(d).all() and np.isfinite(e).all()
    assert np.abs(e - e_ref).max() < 1e-12, w.describe(e - e_ref, K, ns, grid)
    assert np.abs(d - d_ref).max() < 1e-11 * scale, w.describe(d - d_ref, K, ns, grid)
    assert np.abs(xn - e_ref).max() < 1e-12, w.describe(xn - e_ref, K, ns, grid)
    assert np.abs(xn - e).max() < 1e-13, w.describe(xn - e, K, ns, grid)


FLOAT = [
    ("exo", "exo", 4, "exo pcp", "linearize_pcp_kernel<false, float, float, false, 1>"),
    ("aero", "aero", 4, "aero split pcp2", "linearize_pcp2_kernel<true, float, float, false>"),
    ("exo,npts=1", "exo", 1, "exo column-per-lane", "linearize_kernel<false, float>: 16 segments per block, the ragged last block"),
]


@pytest.mark.parametrize("name,model_name,npts,form,what", FLOAT, ids=[c[0] for c in FLOAT])
def test_float_forms_at_the_walk_shape(name, model_name, npts, form, what, aero_tables):
    """(b) scvx_linearize_f32 / scvx_propagate_f32 at the same shape: the stated 2e-5 (endpoint) / 2e-4 (derivative, relative to the
    largest entry of its column) against the fp64 oracle, exactly as tests/test_gpu_discretize.py applies them."""
    from successiveconvexification_amd.dynamics import IntegratorCache, linearize_batch_f32, propagate_batch_f32
    cus, K = _cus(), K13
    B = w.walk_shape(cus, K)
    ns, grid = _walk(form, B * K, cus, 2)
    x, u, sigma, e_ref, d_ref = _reference(model_name, B, K, npts, aero_tables)
    pp = _problems(model_name, aero_tables)[0]
    c = IntegratorCache(pp, npts=npts)
    e32, d32 = linearize_batch_f32(c, x, u, sigma, 1.0 / (K + 1))
    xp32 = propagate_batch_f32(c, x, u, sigma, 1.0 / (K + 1))
    c.close()
    assert e32.dtype == np.float32 and d32.dtype == np.float32
    escale = max(1.0, np.abs(e_ref).max())
    scale = np.abs(d_ref).max(axis=(0, 1, 3), keepdims=True)          # per column of the derivative
    rel = np.abs(d32 - d_ref) / np.maximum(scale, 1.0)
    print("K1 walk float %-12s B %d NS %d: endpoint %.2e  derivative (relative) %.2e  K2 %.2e  K2-K1 %.2e"
          % (name, B, ns, np.abs(e32 - e_ref).max(), rel.max(), np.abs(xp32 - e_ref).max(), np.abs(xp32 - e32).max()))
    assert np.abs(e32 - e_ref).max() < 2e-5 * escale, w.describe(e32 - e_ref, K, ns, grid)
    assert rel.max() < 2e-4, w.describe(rel, K, ns, grid)
    assert np.abs(xp32 - e_ref).max() < 2e-5 * escale, w.describe(xp32 - e_ref, K, ns, grid)
    assert np.abs(xp32 - e32).max() < 2e-6, w.describe(xp32 - e32, K, ns, grid)


# ---- through the batch: the float tile store and the skip list --------------------------------------------------------------------

def _tiles_are_the_linearisation(b, po, npts, f32, ns, grid, what):
    """THE invariant: for every trajectory the batch's endpoint and tiles are the oracle's linearisation of the batch's current
    trajectory.  Double tiles to the bounds of (a); float tiles (double arithmetic, rounded once at the store) within
    2**-24 |d_ref| + 1e-11 max(1, |d_ref|max) per entry.  Returns (endpoint error, largest derivative error / its bound)."""
    from oracle import dynamics as od
    K = b.K
    x, u, s = b.trajectory()
    e, d = b.linearization()
    e_ref, d_ref = od.linearize(od.Params(po), x, u, s, 1.0 / (K + 1), npts)
    scale = max(1.0, np.abs(d_ref).max())
    bound = 1e-11 * scale + (2.0 ** -24 * np.abs(d_ref) if f32 else 0.0)
    ratio = np.abs(d - d_ref) / bound
    assert np.isfinite(d).all() and np.isfinite(e).all(), what
    assert np.abs(e - e_ref).max() < 1e-12, (what, w.describe(e - e_ref, K, ns, grid))
    assert ratio.max() < 1.0, (what, "derivative error / bound: " + w.describe(ratio, K, ns, grid))
    return np.abs(e - e_ref).max(), ratio.max(), np.abs(d - d_ref).max()


def _batch(model_name, npts, f32, aero_tables):
    from oracle import model
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    cus = _cus()
    B = w.walk_shape(cus, K13)
    pp, po, _ = _problems(model_name, aero_tables, K13)
    ic = model.disperse_ics(po, B, 20261018)
    c = IntegratorCache(pp, npts=npts)
    b = ScvxBatch(c, B)
    if f32:
        b.set_linearization_f32(True)
    b.init(ic)
    if model_name != "exo":
        # The straight-line initial guess points the body axis along the velocity, and there the aerodynamic model has no derivative to
        # compare: angle of attack on the edge of its clamp, lift direction 0 / 0.  The two CPU references (C oracle, automatic
        # differentiation) are 1.4e-5 apart on such a node and either moves by 1e-6 under a relative 1e-15 nudge of v, so no bound
        # on |tile - reference| below that means anything.  One common solve_step takes every trajectory off that set (and leaves the
        # left-out ones with a non-trivial state, as test_masked_trajectories_are_left_alone_and_cost_nothing does); bounds unchanged.
        st = b.solve_step()[0]
        assert np.all(st == 1), np.unique(st, return_counts=True)
    return c, b, po, B, cus


@pytest.mark.parametrize("model_name,form", [("exo", "exo pcp"), ("aero+fins", "fins + aero split pcp2")])
def test_float_tile_store_at_the_walk_shape(model_name, form, aero_tables):
    """(b) launch_linearize_store_f32 -- linearize_pcp_kernel<false, double, float, false, 1> and linearize_pcp2_kernel<true, double,
    float, true>, npts = 4: the same walk with 8-byte tile stores of converted pairs.  ScvxBatch.init with set_linearization_f32 at the
    batch's own (dispersed) trajectory: the endpoint stays double (1e-12), every tile entry is the double result rounded once.  The
    aerodynamic batch is compared after one common solve_step (_batch says why): that step's launch_linearize_store_f32, every
    trajectory marked changed, wrote the tiles compared."""
    c, b, po, B, cus = _batch(model_name, 4, True, aero_tables)
    ns, grid = _walk(form, B * K13, cus, 2)
    ee, ratio, de = _tiles_are_the_linearisation(b, po, 4, True, ns, grid, "after init")
    e, d = b.linearization()
    assert np.array_equal(d, d.astype(np.float32).astype(np.float64))      # the tiles are floats
    print("K1 walk float tiles %-10s B %d NS %d: endpoint %.2e  derivative %.2e = %.2f of its bound" % (model_name, B, ns, ee, de, ratio))
    b.close(); c.close()


SKIP = [
    ("exo", "exo", 4, False, {}, "exo pcp",
     "linearize_pcp_kernel<false, ...>: advance() in the producer's and the consumers' walk"),
    ("exo,npts=1", "exo", 1, False, {}, "exo pc",
     "linearize_pc_kernel<false, true, ...>: the early return of a one-group block"),
    ("exo,VARIANT=0", "exo", 4, False, {"SCVX_K1_VARIANT": "0"}, "exo column-per-lane",
     "linearize_kernel<false, double>: the early return of the column-per-lane kernel (16-segment blocks)"),
    ("aero+fins", "aero+fins", 3, False, {}, "fins + aero split pcp2",
     "linearize_pcp2_kernel<true, double, double, true>: its own advance() in P0, P1 and the consumers, NB = 2"),
    ("exo,float tiles", "exo", 4, True, {}, "exo pcp",
     "linearize_pcp_kernel<false, double, float, false, 1>: skipped float tiles stay, recomputed ones are rounded once"),
]


@pytest.mark.parametrize("name,model_name,npts,f32,env,form,what", SKIP, ids=[c[0] for c in SKIP])
def test_skip_list_keeps_tiles_equal_to_the_linearisation_of_the_iterate(name, model_name, npts, f32, env, form, what, aero_tables,
                                                                        monkeypatch):
    """(c) block_unchanged / advance through solve_step, K = 13, dispersed initial conditions.  Two steps under the two masks of
    k1_walk_reference.skip_masks (tests/test_k1_walk_cpu.py: each produces, for this form's NS, a block whose first group is skipped
    and a later one computed, a skipped group between two computed ones, a block that computes nothing and a group that straddles a
    left-out and a stepped trajectory; the ragged last group is skipped under the first and computed under the second).  After each:
    left-out trajectories keep trajectory, endpoint and tiles bit for bit; every accepted step moved its iterate, and at least a third
    of the batch did; and for ALL trajectories the tiles are the oracle's linearisation of the current iterate -- what a wrong skip
    breaks: a group skipped although one of its trajectories moved keeps the tiles of the old iterate, a group mis-walked after a
    skipped one holds another group's inputs.  The aero + fins batch takes one common solve_step before the sequence (_batch says why),
    so its two masked steps are second and third steps; K stays 13: 880 of 1,593 accepted under the first mask, 701 under the second."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c, b, po, B, cus = _batch(model_name, npts, f32, aero_tables)
    ns, grid = _walk(form, B * K13, cus, 2)
    masks = w.skip_masks(B, K13, cus)
    _tiles_are_the_linearisation(b, po, npts, f32, ns, grid, "after init")
    for n, mask in enumerate(masks):
        x0, u0, s0 = b.trajectory()
        e0, d0 = b.linearization()
        b.set_flags(b.flags()[0], mask, mask)
        st, nun, dj = b.solve_step()
        x1, u1, s1 = b.trajectory()
        e1, d1 = b.linearization()
        off, on = mask == 0, mask == 1
        assert np.array_equal(x1[off], x0[off]) and np.array_equal(u1[off], u0[off]) and np.array_equal(s1[off], s0[off]), n
        assert np.array_equal(e1[off], e0[off]) and np.array_equal(d1[off], d0[off]), n
        accepted = on & np.isin(st, (0, 1))                               # SCVX_ST_CONVERGED / SCVX_ST_RUNNING: the candidate became the iterate
        moved = (x1 != x0).any(axis=(1, 2)) | (u1 != u0).any(axis=(1, 2)) | (s1 != s0)
        print("K1 walk skip %-16s step %d: stepped %d of %d, accepted %d, moved %d, statuses %s"
              % (name, n + 1, on.sum(), B, accepted.sum(), moved.sum(), dict(zip(*np.unique(st[on], return_counts=True)))))
        assert moved[accepted].all() and not moved[~accepted].any(), n
        assert 3 * accepted.sum() >= B, (n, accepted.sum(), B)
        kept = ~accepted                                                    # a rejected step keeps its reference point: same tiles
        assert np.array_equal(e1[kept], e0[kept]) and np.array_equal(d1[kept], d0[kept]), n
        ee, ratio, de = _tiles_are_the_linearisation(b, po, npts, f32, ns, grid, "after step %d" % (n + 1))
        print("K1 walk skip %-16s step %d: endpoint %.2e  derivative %.2e = %.2f of its bound" % (name, n + 1, ee, de, ratio))
    b.close(); c.close()
