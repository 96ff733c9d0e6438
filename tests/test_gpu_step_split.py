"""The split solve_step: a batch stepped as M contiguous parts on side streams of the context computes, bit for bit, what the same calls
compute on the context's stream alone (SCVX_STEP_SPLIT=1).  Trajectories never interact, every kernel of the step indexes per trajectory
and the device counters are integer-valued atomic sums, so there is no tolerance anywhere in this file: every comparison is of bytes.
SCVX_STEP_SPLIT = 2 / 3 / 4 forces that many parts at any B >= M (B = 5: 3 + 2, 2 + 2 + 1, 2 + 1 + 1 + 1), with any executor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20261004


def _ics(p, B):
    from successiveconvexification_amd.montecarlo import disperse_ics
    return disperse_ics(p, 0, B, SEED)


def _cache(p=None):
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache
    return IntegratorCache(sp.base_prob_scaled if p is None else p)


def _batch(c, B, **kw):
    from successiveconvexification_amd.batch import ScvxBatch
    return ScvxBatch(c, B, **kw).init(_ics(c.problem, B))


def _parts(b):
    return b._L.scvx_debug_step_parts(b.handle)


def _snap(b):
    """everything a caller can read of a batch, as bytes"""
    st = b.step_stats(reset=False)
    arrs = (b.trajectory_record(),) + b.scalars() + b.flags() + b.solver_stats() + (np.array([st[k] for k in sorted(st)]),)
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrs)


def _env(monkeypatch, split, waves=None):
    monkeypatch.setenv("SCVX_STEP_SPLIT", str(split))
    if waves is None:
        monkeypatch.delenv("SCVX_K4_WAVES", raising=False)
    else:
        monkeypatch.setenv("SCVX_K4_WAVES", str(waves))


def _multi_step(B, every):
    """14 solve_step_async, reset, 3 more; a snapshot after every step (every step then forks again) or only at the end (the
    pipeline never joins on the host)"""
    c = _cache()
    b = _batch(c, B)
    out, parts = [], set()
    for n in range(17):
        if n == 14:
            b.reset()
            parts.add(_parts(b))
        b.solve_step_async()
        parts.add(_parts(b))
        if every:
            out.append(_snap(b))
    out.append(_snap(b))
    b.close(); c.close()
    return out, parts


_REF = {}


def _multi_step_ref(monkeypatch, B, waves, every):
    key = (B, waves, every)
    if key not in _REF:
        _env(monkeypatch, 1, waves)
        _REF[key], parts = _multi_step(B, every)
        assert parts == {1}
    return _REF[key]


@pytest.mark.parametrize("every", [True, False], ids=["read_every_step", "read_at_end"])
@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_multi_step_forced_parts(M, waves, every, monkeypatch):
    ref = _multi_step_ref(monkeypatch, 5, waves, every)
    _env(monkeypatch, M, waves)
    got, parts = _multi_step(5, every)
    assert parts == {M}
    assert got == ref


@pytest.mark.parametrize("M", [2, 3, 4])
def test_multi_step_forced_parts_b7_default_executor(M, monkeypatch):
    ref = _multi_step_ref(monkeypatch, 7, None, False)
    _env(monkeypatch, M)
    got, parts = _multi_step(7, False)
    assert parts == {M}
    assert got == ref


def test_fewer_trajectories_than_parts_runs_unsplit(monkeypatch):
    res = {}
    for split in (1, 4):
        _env(monkeypatch, split)
        c = _cache()
        b = _batch(c, 3)
        for _ in range(3):
            b.solve_step_async()
        assert _parts(b) == 1
        res[split] = _snap(b)
        b.close(); c.close()
    assert res[1] == res[4]


@pytest.mark.parametrize("active", [[1, 0, 1, 1, 0], [1, 1, 1, 0, 0]], ids=["one_inactive_in_each_part", "one_part_all_inactive"])
def test_masked_trajectories(active, monkeypatch):
    res = {}
    for split in (1, 2):      # B = 5 as 3 + 2
        _env(monkeypatch, split)
        c = _cache()
        b = _batch(c, 5)
        b.solve_step_async()
        b.set_flags(active=active)
        for _ in range(3):
            b.solve_step_async()
        assert _parts(b) == split
        res[split] = _snap(b)
        b.close(); c.close()
    assert res[1] == res[2]


def _ordered_calls():
    """calls between steps that the steps must be ordered with; returns the snapshots and the other results along the way"""
    import torch
    c = _cache()
    b = _batch(c, 5)
    out = []
    b.solve_step_async(); b.solve_step_async()
    rk, cost, it = b.scalars()
    b.set_scalars(rk=0.5 * rk)
    b.solve_step_async(); out.append(_snap(b))
    x, u, s = b.trajectory()
    b.set_trajectory(x, u, 1.01 * s)
    b.solve_step_async(); b.solve_step_async(); out.append(_snap(b))
    b.set_thrust_margins(0.01, 0.02)
    b.solve_step_async(); out.append(_snap(b))
    b.solve_step_async()
    out.append(b.flight_check().raw.tobytes())
    b.solve_step_async(); out.append(_snap(b))
    b.solve_step_async()
    out.append(tuple(np.ascontiguousarray(a).tobytes() for a in b.solve()))
    b.reset()
    b.solve_step_async(); b.solve_step_async(); out.append(_snap(b))
    # the caller's own stream: after the step only THAT stream is synchronised, then the iterate is read through the raw device pointer
    ts = torch.cuda.Stream()
    c.set_stream(ts.cuda_stream)
    b.solve_step_async(); b.solve_step_async()
    ptr, n = b.trajectory_dev()

    class _Dev:
        __cuda_array_interface__ = {"shape": (5, n // 5), "typestr": "<f8", "data": (ptr, False), "version": 2}
    view = torch.as_tensor(_Dev(), device="cuda")
    b.solve_step_async()
    ts.synchronize()
    with torch.cuda.stream(ts):
        out.append(view.cpu().numpy().tobytes())
    b.solve_step_async()      # the pointer is out: this batch forks and joins at every step from here on
    ts.synchronize()
    with torch.cuda.stream(ts):
        out.append(view.cpu().numpy().tobytes())
    out.append(_snap(b))
    c.set_stream(None)
    b.solve_step_async(); out.append(_snap(b))
    b.close(); c.close()
    return out


def test_calls_between_steps_are_ordered(monkeypatch):
    _env(monkeypatch, 1)
    ref = _ordered_calls()
    _env(monkeypatch, 2)
    assert _ordered_calls() == ref


def test_two_split_batches_on_one_cache_and_close_without_sync(monkeypatch):
    res = {}
    for split in (1, 2):
        _env(monkeypatch, split)
        c = _cache()
        b1, b2 = _batch(c, 5), _batch(c, 7)
        for n in range(4):
            b1.solve_step_async()
            b2.solve_step_async()
        b3 = _batch(c, 5)
        b3.solve_step_async()
        b3.close()                 # right behind the step, nothing synchronised
        b1.solve_step_async()
        assert _parts(b1) == split and _parts(b2) == split
        res[split] = (_snap(b1), _snap(b2))
        b1.close(); b2.close(); c.close()
    assert res[1] == res[2]


@pytest.mark.parametrize("variant", ["fins", "float_tiles"])
def test_model_variants(variant, monkeypatch):
    from successiveconvexification_amd import sample_problems as sp
    res = {}
    for split in (1, 2):
        _env(monkeypatch, split)
        c = _cache(sp.base_prob_fin_scaled() if variant == "fins" else None)
        assert c.nu == (5 if variant == "fins" else 3)
        b = _batch(c, 5)
        if variant == "float_tiles":
            b.set_linearization_f32(True)
        for _ in range(3):
            b.solve_step_async()
        b.reset()
        b.solve_step_async()
        assert _parts(b) == split
        res[split] = _snap(b)
        b.close(); c.close()
    assert res[1] == res[2]


@pytest.mark.parametrize("split", [1, 2])
def test_profile_of_a_split_step(split, monkeypatch):
    """steps counted once per step however many parts; every class finite, >= 0 and no longer than the region's wall time (events around it
    on the context's stream).  Unsplit the classes are sums of consecutive intervals on one stream, so their total fits in the region too;
    split they are unions over the parts and overlap each other."""
    import torch
    _env(monkeypatch, split)
    c = _cache()
    b = _batch(c, 7)
    ts = torch.cuda.Stream()
    c.set_stream(ts.cuda_stream)
    b.solve_step_async()
    b.set_profiling(True)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(ts)
    for _ in range(3):
        b.solve_step_async()
    t1.record(ts)
    ts.synchronize()
    wall = t0.elapsed_time(t1)
    prof, n = b.profile()
    print("split %d: wall %.4f ms, profile %s" % (split, wall, prof))
    assert _parts(b) == split
    assert n == 3
    for k, v in prof.items():
        assert np.isfinite(v) and 0.0 <= v <= wall, (k, v, wall)
    assert prof["socp"] > 0.0
    if split == 1:
        assert sum(prof.values()) <= wall
    prof2, n2 = b.profile()
    assert n2 == 0 and all(v == 0.0 for v in prof2.values())
    b.set_profiling(False)
    c.set_stream(None)
    b.close(); c.close()


@pytest.mark.parametrize("B,parts", [(2050, 2), (2049, 1)])
def test_default_rule_at_a_real_size(B, parts, monkeypatch):
    """one-wavefront executor, no hint: split when every part has more than 4 x CUs trajectories (256 CUs: B >= 2050)"""
    res = {}
    for split in (None, 1):
        monkeypatch.setenv("SCVX_K4_WAVES", "1")
        if split is None:
            monkeypatch.delenv("SCVX_STEP_SPLIT", raising=False)
        else:
            monkeypatch.setenv("SCVX_STEP_SPLIT", "1")
        c = _cache()
        b = _batch(c, B)
        b.solve_step_async(); b.solve_step_async()
        assert _parts(b) == (parts if split is None else 1)
        res[split] = _snap(b)
        b.close(); c.close()
    assert res[None] == res[1]
