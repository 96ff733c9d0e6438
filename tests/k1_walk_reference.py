"""Host model of K1's group walk (successiveconvexification_amd/csrc/scvx_discretize.hip) -- a helper module, not a test file.

K1 cuts the B * K segments of a batch into groups of NS consecutive segments.  The one-group-per-block kernels launch a block per
group.  The persistent kernels (linearize_pcp_kernel, linearize_pcp2_kernel; from three substeps up) launch
grid = min(ngrp, num_cus * PC_BLOCKS_PER_CU) blocks, and block b walks the groups b, b + grid, b + 2 grid, ...  Under solve_step every
kernel gets the per-trajectory list `skip` and leaves out a group all of whose trajectories are marked unchanged (block_unchanged);
the persistent kernels jump over such groups (advance).  This file restates that walk in plain Python, so that tests can

  * choose a batch at which every persistent form runs more than two groups per block, unevenly, and ends on a ragged group
    (walk_shape),
  * choose masks under which the skip list meets every case of the walk (skip_masks), and
  * say for a segment that came out wrong where in the walk it sat (locate).

Nothing here touches the device; tests/test_k1_walk_cpu.py checks the model by hand-worked cases and against the source text.
"""
import numpy as np

SOURCE = "successiveconvexification_amd/csrc/scvx_discretize.hip"

# constants of the source the table below is made of: (name, value, line, text that line holds)
CONSTANTS = [
    ("WAVES_PER_BLOCK", 4, 24, "constexpr int WAVES_PER_BLOCK = 4;"),
    ("SPW", (4, 3, 2), 35, "SPW = FIN ? 2 : (AERO ? 3 : 4)"),           # segments per wavefront: exo, aero, fins
    ("PC_WAVES", 8, 195, "#define SCVX_PC_WAVES 8"),
    ("PC_BLOCKS_PER_CU", 1, 201, "#define SCVX_PC_BLOCKS_PER_CU 1"),
    ("NB_EXO", 1, 389, "#define SCVX_K1_NB_EXO 1"),
    ("NB", 2, 628, "#define SCVX_K1_NB 2"),                             # segment batches per consumer lane, aero split only (line 630)
]
PC_WAVES, WAVES_PER_BLOCK, PC_BLOCKS_PER_CU = 8, 4, 1
SPW_EXO, SPW_AERO, SPW_FIN = 4, 3, 2

# NS = consumer wavefronts * NB * SPW segments per group.  `line` / `text`: where the kernel of that form computes its NS.
# pcp  = linearize_pcp_kernel  (one producer wavefront, PC_WAVES - 1 = 7 consumers),
# pcp2 = linearize_pcp2_kernel (producer split over two wavefronts, PC_WAVES - 2 = 6 consumers; NB = 2 with aerodynamics),
# pc   = linearize_pc_kernel   (one group per block, 7 consumers), column-per-lane = linearize_kernel (4 wavefronts, no producer).
FORMS = {
    # persistent
    "exo pcp":                       dict(ns=7 * 1 * 4, persistent=True, line=402, text="constexpr int NS = NC * SPW * NB;"),
    "aero split pcp2":               dict(ns=6 * 2 * 3, persistent=True, line=643, text="constexpr int NS = NC * SPW * NB;"),
    "fins + aero split pcp2":        dict(ns=6 * 2 * 2, persistent=True, line=643, text="constexpr int NS = NC * SPW * NB;"),
    "fins exo split pcp2":           dict(ns=6 * 1 * 2, persistent=True, line=643, text="constexpr int NS = NC * SPW * NB;"),
    "aero + torque pcp (SG=0)":      dict(ns=7 * 1 * 3, persistent=True, line=402, text="constexpr int NS = NC * SPW * NB;"),
    "fins (+ torque) pcp (SG=0)":    dict(ns=7 * 1 * 2, persistent=True, line=402, text="constexpr int NS = NC * SPW * NB;"),
    # one group per block
    "exo pc":                        dict(ns=7 * 4, persistent=False, line=244, text="constexpr int NS = NC * SPW;"),
    "aero pc":                       dict(ns=7 * 3, persistent=False, line=244, text="constexpr int NS = NC * SPW;"),
    "fins pc":                       dict(ns=7 * 2, persistent=False, line=244, text="constexpr int NS = NC * SPW;"),
    "exo column-per-lane":           dict(ns=4 * 4, persistent=False, line=67, text="WAVES_PER_BLOCK * SPW"),
    "aero column-per-lane":          dict(ns=4 * 3, persistent=False, line=67, text="WAVES_PER_BLOCK * SPW"),
}
NS_MAX = max(f["ns"] for f in FORMS.values())
PERSISTENT_NS = sorted({f["ns"] for f in FORMS.values() if f["persistent"]})
ALL_NS = sorted({f["ns"] for f in FORMS.values()})


def ngrp_of(nseg, ns):
    return (nseg + ns - 1) // ns


def grid_of(nseg, ns, cus, persistent=True):
    """launch_linearize_t: a block per group, capped at one block per CU for the persistent kernels"""
    n = ngrp_of(nseg, ns)
    return min(n, cus * PC_BLOCKS_PER_CU) if persistent else n


def block_unchanged(skip, seg0, nseg_block, nseg, K):
    """block_unchanged of the source: every trajectory that owns one of the segments seg0 .. seg0 + nseg_block - 1 (cut at nseg) is
    marked.  skip: per trajectory, true = unchanged; None = no list (the direct entry points)."""
    if skip is None or seg0 >= nseg:
        return False
    seg1 = min(seg0 + nseg_block - 1, nseg - 1)
    for b in range(seg0 // K, seg1 // K + 1):
        if not skip[b]:
            return False
    return True


def groups_of_block(nseg, K, ns, grid, skip=None):
    """The groups each of the `grid` blocks computes, in the order it computes them: block b starts at advance(b) and goes on at
    advance(g + grid).  grid = ngrp gives the one-group-per-block kernels (a block computes its group or returns at once)."""
    ngrp = ngrp_of(nseg, ns)

    def advance(g):
        while g < ngrp and block_unchanged(skip, g * ns, ns, nseg, K):
            g += grid
        return g

    out = []
    for b in range(grid):
        mine = []
        g = advance(b)
        while g < ngrp:
            mine.append(g)
            g = advance(g + grid)
        out.append(mine)
    return out


def walk_shape(cus, K, rounds=2):
    """Smallest B at which (1) the form with the largest groups has ngrp >= rounds * cus + cus / 4 -- some blocks walk rounds + 1
    groups and the rest `rounds`, so block loads are uneven -- and (2) B * K is no multiple of any NS of the table, so every form ends
    on a ragged group."""
    need = rounds * cus + cus // 4
    B = max(1, ((need - 1) * NS_MAX) // K)
    while ngrp_of(B * K, NS_MAX) < need or any((B * K) % ns == 0 for ns in ALL_NS):
        B += 1
    return B


def locate(seg, ns, grid):
    """(group, round, place in the group) of a segment for a form with `ns` segments per group walked by `grid` blocks"""
    g = seg // ns
    return g, g // grid, seg % ns


def describe(err, K, ns, grid):
    """for an assertion message: where in the walk the largest entry of err [B][K][...] sits"""
    flat = np.abs(err).reshape(err.shape[0] * err.shape[1], -1)
    seg = int(flat.max(axis=1).argmax())
    col = int(flat[seg].argmax())
    g, r, j = locate(seg, ns, grid)
    return ("worst %.3e at segment %d (trajectory %d, node %d), group %d = round %d of block %d, place %d of %d, flat column %d"
            % (flat[seg, col], seg, seg // K, seg % K, g, r, g % grid, j, ns, col))


# ---- the skip list -------------------------------------------------------------------------------------------------------------------

def walk_cases(nseg, K, ns, grid, skip):
    """Which of the cases of the walk a mask (true = left out) produces for one form.  Returns a dict of counts:
    first_skipped  blocks whose first group is skipped and a later one computed,
    hole           blocks with a skipped group between two computed ones,
    all_skipped    blocks that have groups and compute none,
    straddle       groups that hold a left-out and a stepped trajectory (they are computed),
    last_skipped   1 if the ragged last group is skipped."""
    ngrp = ngrp_of(nseg, ns)
    unchanged = [block_unchanged(skip, g * ns, ns, nseg, K) for g in range(ngrp)]
    res = dict(first_skipped=0, hole=0, all_skipped=0, straddle=0, last_skipped=int(unchanged[-1]))
    for g in range(ngrp):
        b0, b1 = (g * ns) // K, min((g + 1) * ns - 1, nseg - 1) // K
        n = sum(1 for b in range(b0, b1 + 1) if skip[b])
        if 0 < n < b1 - b0 + 1:
            assert not unchanged[g]
            res["straddle"] += 1
    for b in range(grid):
        f = unchanged[b::grid]
        if not f:
            continue
        if all(f):
            res["all_skipped"] += 1
            continue
        if f[0]:
            res["first_skipped"] += 1
        first, last = f.index(False), len(f) - 1 - f[::-1].index(False)
        if any(f[first:last + 1]):
            res["hole"] += 1
    return res


def _cases_ok(nseg, K, cus, left):
    for f in FORMS.values():
        grid = grid_of(nseg, f["ns"], cus, f["persistent"])
        c = walk_cases(nseg, K, f["ns"], grid, left)
        if not (c["all_skipped"] and c["straddle"]):
            return False
        if f["persistent"] and not (c["first_skipped"] and c["hole"]):
            return False
    return True


def _runs(rng, left, allowed, target, B):
    """mark runs of consecutive trajectories inside `allowed` until `target` of them are marked: short runs (a group or less) and long
    ones (many groups), so that groups fall wholly inside, wholly outside and across the edges"""
    long_hi = max(12, B // 12)
    for _ in range(100000):
        if left.sum() >= target:
            break
        n = int(rng.integers(2, 7)) if rng.random() < 0.5 else int(rng.integers(8, long_hi + 1))
        a = int(rng.integers(0, B))
        sel = np.arange(a, min(B, a + n))
        left[sel[allowed[sel]]] = True


def _comb(rng, left, nseg, K, cus):
    """for every persistent NS one block all of whose groups are left out, rounds included that no run would hit together"""
    for ns in PERSISTENT_NS:
        grid = grid_of(nseg, ns, cus)
        b = int(rng.integers(0, grid))
        for g in range(b, ngrp_of(nseg, ns), grid):
            left[(g * ns) // K: min((g + 1) * ns - 1, nseg - 1) // K + 1] = True


def skip_masks(B, K, cus, tries=200):
    """Two masks (int32 [B], 1 = stepped, 0 = left out; what set_flags takes as `active`) for the skip-list tests.  Each produces, for
    every form of the table at grid = min(ngrp, cus), every case walk_cases counts (first_skipped and hole only where a block walks
    more than one group: the persistent forms).  The first leaves the tail of the batch out, so the ragged last group of every form
    is skipped; the second steps it.  Each steps at least a third and leaves out at least a quarter, and at least a third of the
    batch is left out by the first and stepped by the second: for those the second solve_step is their first, which the trust-region
    rule always accepts (the cost before it is infinite), so the count of moved iterates cannot depend on the problem.
    Deterministic: seeds are tried in order until the model confirms all of it."""
    nseg = B * K
    tail = -(-NS_MAX // K) + 1
    for seed in range(tries):
        rng = np.random.default_rng(20261018 + seed)
        left1 = np.zeros(B, bool)
        _runs(rng, left1, np.ones(B, bool), int(0.42 * B), B)
        _comb(rng, left1, nseg, K, cus)
        left1[B - tail:] = True
        left2 = np.zeros(B, bool)
        _runs(rng, left2, ~left1, int(0.27 * B), B)
        _comb(rng, left2, nseg, K, cus)
        left2[B - 1] = False
        ok = (3 * (~left1).sum() >= B and 3 * (~left2).sum() >= B and 4 * left1.sum() >= B and 4 * left2.sum() >= B
              and 3 * (left1 & ~left2).sum() >= B)
        if ok and _cases_ok(nseg, K, cus, left1) and _cases_ok(nseg, K, cus, left2):
            return (~left1).astype(np.int32), (~left2).astype(np.int32)
    raise ValueError("no pair of masks with the required cases at B = %d, K = %d, %d CUs" % (B, K, cus))
