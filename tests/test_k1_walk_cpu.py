"""tests/k1_walk_reference.py, the host model of K1's persistent group walk and skip list, checked without a GPU: its table against the
text of the kernel source, the model on cases small enough to work by hand, the shape it picks, and that the two masks it makes for
tests/test_gpu_k1_walk.py produce every case of the walk for every kernel form."""
import os
import re

import numpy as np
import pytest

import k1_walk_reference as w
from conftest import ROOT

CUS = (32, 64, 256, 304)


def test_table_points_at_the_source():
    """Every entry's line holds the text it names, and the constants the table is made of are the source's."""
    with open(os.path.join(ROOT, w.SOURCE)) as f:
        lines = f.read().split("\n")
    for name, value, line, text in w.CONSTANTS:
        assert text in lines[line - 1], (name, line, lines[line - 1])
    for name, f in w.FORMS.items():
        assert f["text"] in lines[f["line"] - 1], (name, f["line"], lines[f["line"] - 1])
    src = "\n".join(lines)
    assert int(re.search(r"#define SCVX_PC_WAVES (\d+)", src).group(1)) == w.PC_WAVES == 8
    assert int(re.search(r"constexpr int WAVES_PER_BLOCK = (\d+);", src).group(1)) == w.WAVES_PER_BLOCK == 4
    assert int(re.search(r"#define SCVX_PC_BLOCKS_PER_CU (\d+)", src).group(1)) == w.PC_BLOCKS_PER_CU == 1
    assert re.search(r"#define SCVX_K1_NB (\d+)", src).group(1) == "2" and re.search(r"#define SCVX_K1_NB_EXO (\d+)", src).group(1) == "1"
    assert "NB = AERO ? SCVX_K1_NB : 1" in lines[630 - 1]
    assert (w.SPW_EXO, w.SPW_AERO, w.SPW_FIN) == (4, 3, 2)
    ns = {k: f["ns"] for k, f in w.FORMS.items()}
    assert ns == {"exo pcp": 28, "aero split pcp2": 36, "fins + aero split pcp2": 24, "fins exo split pcp2": 12,
                  "aero + torque pcp (SG=0)": 21, "fins (+ torque) pcp (SG=0)": 14,
                  "exo pc": 28, "aero pc": 21, "fins pc": 14, "exo column-per-lane": 16, "aero column-per-lane": 12}
    assert w.PERSISTENT_NS == [12, 14, 21, 24, 28, 36] and w.NS_MAX == 36
    # a block meets a second group only above cap * NS segments
    assert [256 * n for n in (28, 36, 24, 12)] == [7168, 9216, 6144, 3072]


def test_model_on_hand_worked_cases():
    # 1. no list: 10 segments, groups of 3 -> groups 0..3 (the last holds one segment), two blocks take them alternately
    assert w.groups_of_block(10, 5, 3, 2) == [[0, 2], [1, 3]]
    # 2. the same walk, trajectory 0 of two (K = 5: segments 0..4) left out.  Group 0 = segments 0..2: skipped.  Group 1 = segments 3..5
    #    straddles trajectories 0 and 1: computed.  Groups 2, 3 belong to trajectory 1: computed.
    assert w.groups_of_block(10, 5, 3, 2, [True, False]) == [[2], [1, 3]]
    # 3. trajectory 1 left out instead: group 2 (segments 6..8) and the ragged group 3 (segment 9) are skipped
    assert w.groups_of_block(10, 5, 3, 2, [False, True]) == [[0], [1]]
    # 4. K = 2, six trajectories, 12 segments, groups of 2 = one trajectory each, two blocks: block 0 has groups 0, 2, 4, block 1 has
    #    1, 3, 5.  Left out: 0, 2 (block 0's first two, its third computed), 3 (between block 1's computed 1 and 5)
    assert w.groups_of_block(12, 2, 2, 2, [True, False, True, True, False, False]) == [[4], [1, 5]]
    # 5. one group per block (grid = ngrp): a block computes its own group or nothing; everything left out -> nothing anywhere
    assert w.groups_of_block(12, 2, 4, 3, [False, False, True, True, False, True]) == [[0], [], [2]]
    assert w.groups_of_block(12, 2, 4, 3, [True] * 6) == [[], [], []]
    # block_unchanged at the edges: a range past the end is never "unchanged" (the kernel's seg0 >= nseg), the last group is cut at nseg
    assert not w.block_unchanged([True], 5, 3, 5, 5) and w.block_unchanged([False, True], 9, 3, 10, 5)
    assert not w.block_unchanged(None, 0, 3, 10, 5)
    # the cases of case 4 as walk_cases names them: block 0 = first_skipped, block 1 = hole
    c = w.walk_cases(12, 2, 2, 2, [True, False, True, True, False, False])
    assert c == dict(first_skipped=1, hole=1, all_skipped=0, straddle=0, last_skipped=0)
    c = w.walk_cases(10, 5, 3, 2, [False, True])
    assert c == dict(first_skipped=0, hole=0, all_skipped=0, straddle=1, last_skipped=1)
    assert w.locate(9, 3, 2) == (3, 1, 0)


@pytest.mark.parametrize("cus", CUS)
def test_walk_shape_has_the_stated_properties(cus):
    K = 13
    B = w.walk_shape(cus, K)
    nseg = B * K
    for b in (B, B - 1):
        ok = w.ngrp_of(b * K, 36) >= 2 * cus + cus // 4 and all((b * K) % ns for ns in w.ALL_NS)
        assert ok == (b == B)                                      # B qualifies; B - 1 does not.  And nothing below it does:
    assert not any(w.ngrp_of(b * K, 36) >= 2 * cus + cus // 4 and all((b * K) % ns for ns in w.ALL_NS) for b in range(1, B))
    # at the largest NS some blocks walk three groups and the rest two; every other persistent form walks at least as many
    walks = [len(g) for g in w.groups_of_block(nseg, K, 36, cus)]
    assert set(walks) == {2, 3} and walks.count(3) >= cus // 4
    for ns in w.PERSISTENT_NS:
        assert min(len(g) for g in w.groups_of_block(nseg, K, ns, cus)) >= 2 and nseg % ns


def test_walk_shape_at_256_cus():
    """The device tests stay small: below 25,000 segments at 256 CUs (a condition, not a measurement).  B = 1631, the shape worked by
    hand when these tests were specified, meets both conditions too (remainders 7 / 35 / 11 / 11 / 14 / 7, ngrp(36) = 589 = 2 * 256 +
    77); the smallest B that does is 1593."""
    assert w.walk_shape(256, 13) == 1593 and 1593 * 13 < 25000
    assert [1631 * 13 % ns for ns in (28, 36, 24, 12, 21, 14)] == [7, 35, 11, 11, 14, 7] and w.ngrp_of(1631 * 13, 36) == 589
    for K in (1, 13, 100):
        assert w.walk_shape(256, K) * K < 25000
    assert w.walk_shape(256, 100) == 209
    B1 = w.walk_shape(256, 13, rounds=1)                           # the shape of the two torque cases
    assert w.ngrp_of(B1 * 13, 36) >= 256 + 64 and all((B1 * 13) % ns for ns in w.ALL_NS)


@pytest.mark.parametrize("cus", CUS)
def test_masks_produce_every_case_of_the_walk_for_every_form(cus):
    K = 13
    B = w.walk_shape(cus, K)
    nseg = B * K
    m1, m2 = w.skip_masks(B, K, cus)
    assert m1.dtype == np.int32 and m1.shape == (B,) and set(np.unique(m1)) == {0, 1} and not np.array_equal(m1, m2)
    a1, a2 = w.skip_masks(B, K, cus)
    assert np.array_equal(a1, m1) and np.array_equal(a2, m2)      # deterministic
    for name, f in w.FORMS.items():
        grid = w.grid_of(nseg, f["ns"], cus, f["persistent"])
        assert grid == (min(w.ngrp_of(nseg, f["ns"]), cus) if f["persistent"] else w.ngrp_of(nseg, f["ns"]))
        last = []
        for m in (m1, m2):
            left = m == 0
            c = w.walk_cases(nseg, K, f["ns"], grid, left)
            assert c["all_skipped"] >= 1 and c["straddle"] >= 1, (name, c)
            if f["persistent"]:       # a block of the other kernels has one group: it cannot skip one and compute another
                assert c["first_skipped"] >= 1 and c["hole"] >= 1, (name, c)
            last.append(c["last_skipped"])
            # walk_cases agrees with the walk written out: the computed groups are exactly those with a stepped trajectory
            walk = w.groups_of_block(nseg, K, f["ns"], grid, left)
            done = sorted(g for b in walk for g in b)
            want = [g for g in range(w.ngrp_of(nseg, f["ns"]))
                    if not left[(g * f["ns"]) // K: min((g + 1) * f["ns"] - 1, nseg - 1) // K + 1].all()]
            assert done == want, name
            assert all(g % grid == b for b, gs in enumerate(walk) for g in gs) and all(gs == sorted(gs) for gs in walk)
            assert sum(1 for gs in walk if not gs) >= c["all_skipped"] >= 1
        assert last == [1, 0], name                                 # the ragged last group: skipped under the first mask, computed under the second
    for m in (m1, m2):
        assert 3 * m.sum() >= B and 4 * (m == 0).sum() >= B          # at least a third stepped, at least a quarter left out
    assert ((m1 == 0) & (m2 == 1)).any()
    # more than the specification asks: a third of the batch takes its FIRST step under the second mask (always accepted)
    assert 3 * ((m1 == 0) & (m2 == 1)).sum() >= B


def test_describe_names_the_place_in_the_walk():
    err = np.zeros((4, 5, 3, 2))
    err[2, 3, 1, 0] = -7.0                                            # segment 13 -> group 4 of 3-segment groups, round 2 of block 0
    s = w.describe(err, 5, 3, 2)
    assert "segment 13 (trajectory 2, node 3), group 4 = round 2 of block 0, place 1 of 3, flat column 2" in s and "7.000e+00" in s
