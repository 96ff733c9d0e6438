"""The cases of test_horizons_cpu.py and test_gpu_horizons.py: the analysis calls at horizons other than the sample problem's K = 50.

Short horizons (K = 1, 2, 3) take random-but-physical plans (conftest.random_segments; no solve is involved); the long one (K = 100)
takes, where a device exists, the recipe of test_gpu_flight._case -- a dispersed batch after three solve_steps -- and random segments
where none does.  B = 3 throughout.  Nothing here is taken from a result of the code under test.
"""
from dataclasses import replace

import numpy as np

from conftest import random_segments

B = 3
SHORT = (1, 2, 3)
LONG = 100
HORIZONS = SHORT + (LONG,)
MODELS = ("exo", "aero+fins")
FLIGHT_ONLY_MODEL = "aero+fins+torque"
FIN_SPAN = 1e-3            # the sample's finmxf is 0.01
# the sampled closed-loop dispersion (test_mc_horizons_cpu.py, test_gpu_mc_horizons.py): K = 3 is pinned by the modules of the calls
MC_HORIZONS = (1, 2, LONG)
MC_SHORT = (1, 2)
MC_S, MC_S_BLOCKS = 5, 130  # the CPU-chain parities; three blocks per plan, the last with two live lanes
MC_SEED = 31                # of the impulse parities, whose count comparison test_mc_horizons_cpu.py vets
_CASES = {}


def mc_nsub(K):
    """substeps per segment of the sampled-dispersion cases: the long horizon's reference chain stays within seconds"""
    return 4 if K == LONG else 2


def problems(model, K, tables):
    """test_gpu_flight._problems at horizon K: (product problem, oracle problem, dyn module of the reference, its Params)"""
    from test_gpu_flight import _problems
    pp, po, dyn, _ = _problems(model, tables)
    pp, po = replace(pp, K=K), replace(po, K=K)
    par = dyn.Params(po, torque=True) if "torque" in model else dyn.Params(po)
    return pp, po, dyn, par


def _segments(po, nu, K, seed):
    x, u, s = random_segments(po, B, K, seed)
    if nu == 5:
        fins = np.random.default_rng(seed + 1).uniform(-FIN_SPAN, FIN_SPAN, (B, K + 1, 2))
        u = np.concatenate([u, fins], axis=-1)
    return x, u, s


def case(model, K, tables, device=False):
    """(pp, po, dyn, par, x, u, sigma) of a model name and a horizon.  device: K = 100 comes from three solve_steps on the device"""
    key = (model, K, bool(device and K == LONG))
    if key not in _CASES:
        pp, po, dyn, par = problems(model, K, tables)
        nu = 5 if "fins" in model else 3
        if key[2]:
            from oracle import model as om
            from successiveconvexification_amd.batch import ScvxBatch
            from successiveconvexification_amd.dynamics import IntegratorCache
            c = IntegratorCache(pp, npts=10)
            b = ScvxBatch(c, B).init(om.disperse_ics(po, B, 20261016))
            for _ in range(3):
                st, _, _ = b.solve_step()
                assert np.isin(st, (0, 1, 2)).all(), st
            xus = b.trajectory()
            b.close()
            c.close()
        else:
            xus = _segments(po, nu, K, 20261020 + K)
        assert xus[0].shape == (B, K + 1, 14) and xus[1].shape == (B, K + 1, nu)
        _CASES[key] = (pp, po, dyn, par) + tuple(xus)
    return _CASES[key]


def flyable_batch(K, steps=3, tiles_f32=False):
    """(cache, batch): the B = 2 dispersed flyable batch (mdry = 0.55, tf_guess = 8) at horizon K after `steps` solve_steps; the caller
    closes both"""
    import bench
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    from test_gpu_flight import _flyable
    pp = replace(_flyable()[0], K=K)
    c = IntegratorCache(pp, npts=10)
    b = ScvxBatch(c, 2).set_linearization_f32(tiles_f32).init(bench.disperse_ics(pp, 0, 2, 7))
    for _ in range(steps):
        st, _, _ = b.solve_step()
        assert np.isin(st, (0, 1, 2)).all(), st
    return c, b
