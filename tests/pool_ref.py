"""The pooled records of a tied batch (csrc/batch_pool.hpp, include/cpprob_hip.h: cpprob_hip_batch_pool_stats) restated in plain Python:
for a group with the members b_0 < b_1 < ..., every entry is (((0.0 + rec[b_0]) + rec[b_1]) + ...), one Python-float addition a member.
pool_exact gives the same sums in fractions, where no order matters.  case() is the tie and the records the kernel-text test and
tests/test_gpu_batch_pool.py share.  The reference of tests/test_pool_ref_host.py and of both of those."""
import os
import re
from fractions import Fraction

import numpy as np

RECORD = 88
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "csrc", "batch_pool.hpp")


def pool_ahead():
    """kPoolAhead as csrc/batch_pool.hpp names it."""
    m = re.search(r"^constexpr int kPoolAhead = (\d+);", open(HEADER).read(), re.M)
    assert m, "kPoolAhead is a named constant"
    return int(m.group(1))


def members(groups):
    """[G] lists: every group's problems in ascending order."""
    groups = [int(g) for g in groups]
    G = max(groups) + 1
    out = [[b for b, g in enumerate(groups) if g == gg] for gg in range(G)]
    assert min(groups) >= 0 and all(out), "ids 0 .. G-1, every one used"
    return out


def pool(rec, groups, broadcast=True, descending=False):
    """rec [B, ...] -> [B, ...] (broadcast) or [G, ...]; descending: the members added in the opposite order (to show that the
    fixtures see the order)."""
    rec = np.asarray(rec, np.float64)
    flat = rec.reshape(rec.shape[0], -1)
    mem = members(groups)
    rows = []
    for grp in mem:
        order = grp[::-1] if descending else grp
        row = []
        for e in range(flat.shape[1]):
            acc = 0.0
            for b in order:
                acc = acc + float(flat[b, e])
            row.append(acc)
        rows.append(row)
    pooled = np.array(rows, np.float64).reshape((len(mem),) + rec.shape[1:])
    return pooled[np.asarray(groups, np.int64)] if broadcast else pooled


def pool_exact(rec, groups):
    """[G][entries] Fractions: the groups' exact sums."""
    flat = np.asarray(rec, np.float64).reshape(len(groups), -1)
    return [[sum((Fraction(float(flat[b, e])) for b in grp), Fraction(0)) for e in range(flat.shape[1])] for grp in members(groups)]


def case_groups(ahead=None):
    """B = 40 problems in groups of 1, A - 1, A, A + 1, 2 A + 3 and the rest (A = kPoolAhead), the memberships interleaved."""
    A = pool_ahead() if ahead is None else int(ahead)
    sizes = [1, A - 1, A, A + 1, 2 * A + 3]
    assert all(s >= 1 for s in sizes) and sum(sizes) < 40
    sizes.append(40 - sum(sizes))
    ids = np.concatenate([np.full(s, g, np.int32) for g, s in enumerate(sizes)])
    groups = np.random.default_rng(4040).permutation(ids).astype(np.int32)
    return groups, sizes


def case(R, seed):
    """(groups int32 [40], records [40, R, 88]): magnitudes over 2^-30 .. 2^30, mixed signs in every entry, 64 .. 87 included."""
    groups, _ = case_groups()
    rng = np.random.default_rng(seed)
    shape = (groups.size, R, RECORD)
    rec = rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(-30, 31, shape).astype(np.float64)) * rng.choice([-1.0, 1.0], shape)
    return groups, rec
