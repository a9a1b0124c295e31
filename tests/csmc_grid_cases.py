"""The batches tests/test_gpu_batch_csmc_grid.py and tests/test_csmc_grid_cases_host.py share: shapes at which batch_csmc_kernel
(csrc/batch_csmc.hpp) walks many steps, many workgroups and the edges of its integer statement, on k = 8 states.  A case is
(k, Ts, ns, means, trans, observes, seeds, paths): means [B, k] and trans [B, k, k] of a described batch, [1, k] and [1, k, k] of a
uniform one (a shared table); paths a list of integer arrays, problem b's reference path.  No test lives here.

Every case and every reference is computed once a process and shared: leave the arrays as they are."""
import functools

import numpy as np

import backward_ref as R
import csmc_ref as CS
from test_gpu_batch_csmc import _observes, _paths, _seeds, _tables

TILE = 256                                                       # kTrajStatsTile
LONG_DRAW = 65535                                                # the largest draw_index

# LONG: a walk of 1500 steps, lengths on both sides of the wavefront (63 / 64 / 65), of two of them (129) and of the rows the backward
# smoother stages in LDS (512 / 513); n from 1 past a pass of 1024 to the count-field limit 8192.  Table 1 has a zero entry (_tables).
LONG_K = 8
LONG_TS = [1500, 1, 63, 64, 65, 129, 512, 513, 2]
LONG_NS = [9, 8192, 70, 3, 300, 65, 16, 5, 1025]

# MANY: more problems than compute units (256), no two neighbours of one length, one problem of two passes.
MANY_K, MANY_B = 8, 300

# ONE_HOT: means 6 apart (a state two levels from the observe has integer weight 0), state 1 absorbing, 0 -> 7 impossible.
ONE_HOT_K, ONE_HOT_T, ONE_HOT_NS = 8, 40, [1, 2, 300]
ONE_HOT_SEED = 3

SEED_VALUES = [0, (1 << 64) - 1, 1 << 63, 1 << 32]

BYTES_TS, BYTES_NS = [7, 1, 64], [5, 300, 64]

# The statistics grid (tests/test_gpu_batch_trajstats_grid.py): T = 512 is the longest problem batch_traj_stats_kernel stages in LDS
# (kBackwardLdsMax = 32768 bytes of 64 a step), T = 513 the shortest it reads from memory.
STATS_TS, STATS_NS = [1, 2, 7, 512, 513], [1, 3, 70, 64, 9]
STATS_SHORT = 3                                                  # the problems of the short batch: T = 1, 2, 7


@functools.lru_cache(maxsize=None)
def long_case():
    means, trans = _tables(LONG_K, len(LONG_TS), 211)
    assert trans[1, 0, LONG_K - 1] == 0.0
    return LONG_K, list(LONG_TS), list(LONG_NS), means, trans, _observes(means, LONG_TS, 212), _seeds(len(LONG_TS), 213), _paths(LONG_K, LONG_TS, 214)


def long_case_cut(T_cut=129):
    """LONG with its two longest problems cut to T_cut steps: the host program's barrier costs far more than the device's."""
    k, Ts, ns, means, trans, obs, seeds, paths = long_case()
    longest = sorted(range(len(Ts)), key=lambda b: -Ts[b])[:2]
    Ts = [min(T, T_cut) if b in longest else T for b, T in enumerate(Ts)]
    return k, Ts, ns, means, trans, [o[:T] for o, T in zip(obs, Ts)], seeds, [p[:T] for p, T in zip(paths, Ts)]


def many_lengths(B=MANY_B, reverse=False):
    Ts = [1 + (7 * b) % 23 for b in range(B)]
    ns = [1 + (5 * b) % 11 for b in range(B)]
    ns[17] = 1025
    assert all(Ts[b] != Ts[b + 1] for b in range(B - 1))
    return (Ts[::-1] if reverse else Ts), ns


def dispatch_order(Ts, ns):
    """The host code's order[]: the longest chains (steps times passes of 1024 particles) first, ties by index."""
    cost = [T * (-(-n // 1024)) for T, n in zip(Ts, ns)]
    return sorted(range(len(Ts)), key=lambda b: -cost[b])


@functools.lru_cache(maxsize=None)
def many_case(B=MANY_B, reverse=False):
    """reverse: the same particle counts over the lengths reversed, with observes and paths of its own."""
    Ts, ns = many_lengths(B, reverse)
    means, trans = _tables(MANY_K, B, 221)
    trans[1::5, 0, MANY_K - 1] = 0.0
    tag = 7 * B + (1 if reverse else 0)
    order = dispatch_order(Ts, ns)
    assert sum(1 for i, b in enumerate(order) if i != b) >= B - 10, "workgroup i should run another problem than i almost everywhere"
    return MANY_K, Ts, ns, means, trans, _observes(means, Ts, 222 + tag), _seeds(B, 223 + tag), _paths(MANY_K, Ts, 224 + tag)


@functools.lru_cache(maxsize=None)
def one_hot_case():
    k, B, T = ONE_HOT_K, len(ONE_HOT_NS), ONE_HOT_T
    rng = np.random.default_rng(ONE_HOT_SEED)
    means = np.tile(6.0 * np.arange(k), (B, 1))
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    trans[:, 1, :] = 0.0
    trans[:, 1, 1] = 1.0
    trans[:, 0, k - 1] = 0.0
    Ts = [T] * B
    case = (k, Ts, list(ONE_HOT_NS), means, trans, _observes(means, Ts, ONE_HOT_SEED + 1), _seeds(B, 231), _paths(k, Ts, ONE_HOT_SEED + 2))
    # the edges the case is for, on the n = 300 problem: without them it would pass on inputs that miss them
    xs, m = states(case, 2)
    occupied = np.array([np.bincount(x, minlength=k) > 0 for x in xs])
    nonzero = np.array(m) > 0
    lone = int(np.sum((nonzero.sum(axis=1) == 1) & (occupied.sum(axis=1) > 1)))
    starved = int(np.sum(occupied & ~nonzero))
    assert lone >= 1, "no row of the n = 300 problem has exactly one non-zero mass under several occupied states"
    assert starved >= 1, "no occupied state of the n = 300 problem has mass 0"
    return case


@functools.lru_cache(maxsize=None)
def seeds_case():
    """A uniform batch: one shared table, every problem T = 5 and n = 257."""
    k, B, T, n = 3, len(SEED_VALUES), 5, 257
    means, trans = _tables(k, 1, 241)
    Ts = [T] * B
    return k, Ts, [n] * B, means, trans, _observes(np.repeat(means, B, 0), Ts, 242), np.array(SEED_VALUES, np.uint64), _paths(k, Ts, 243)


@functools.lru_cache(maxsize=None)
def bytes_case(k):
    """Reference bytes over the whole int8 range: the device form takes the low three bits, and a value >= k as k - 1."""
    B = len(BYTES_TS)
    means, trans = _tables(k, B, 250 + k)
    rng = np.random.default_rng(260 + k)
    paths = [rng.integers(-128, 128, T).astype(np.int8) for T in BYTES_TS]
    flat = np.concatenate(paths).astype(np.int64)
    assert flat.min() < 0 and flat.max() > 7 and np.any((flat & 7) >= k) and np.any((flat & 7) < k - 1)
    assert all(np.any(p < 0) or np.any(p >= k) for p in paths)
    return k, list(BYTES_TS), list(BYTES_NS), means, trans, _observes(means, BYTES_TS, 270 + k), _seeds(B, 280 + k), paths


@functools.lru_cache(maxsize=None)
def stats_case(k, short=False):
    """(k, Ts, ns, means, trans, observes, seeds) of the statistics grid: described problems, a table each; short: the problems of
    at most 7 steps alone."""
    B = STATS_SHORT if short else len(STATS_TS)
    Ts, ns = STATS_TS[:B], STATS_NS[:B]
    means, trans = _tables(k, B, 290 + k)
    return k, Ts, ns, means, trans, _observes(means, Ts, 291 + k), _seeds(B, 292 + k)


def table(case, b):
    """(means [k], trans [k, k]) of problem b: its own, or the shared one."""
    return case[3][b % len(case[3])], case[4][b % len(case[4])]


_STATES, _TRAJ = {}, {}


def states(case, b):
    """csmc_ref.states of problem b (the generations and their integer masses), computed once."""
    k, Ts, ns, _, _, obs, seeds, paths = case
    means, trans = table(case, b)
    key = (means.tobytes(), trans.tobytes(), obs[b].tobytes(), int(seeds[b]), int(ns[b]), np.asarray(paths[b], np.int64).tobytes())
    if key not in _STATES:
        _STATES[key] = CS.states(R.log_likelihoods(obs[b], means), R.thresholds(trans), int(seeds[b]), int(ns[b]), paths[b])
    return _STATES[key]


def want(case, b):
    """(rows [T, 8] float64, the integer masses [T][k], P) of problem b."""
    k = case[0]
    m = states(case, b)[1]
    rows = np.zeros((len(m), 8))
    rows[:, :k] = np.array(m, np.float64)
    return rows, m, R.transition_masses(table(case, b)[1])


def trajectories(case, b, n_traj, draw_index=0):
    """backward_ref.trajectories_fast [T, n_traj] on the reference masses of problem b, computed once."""
    key = (id(case), b, n_traj, draw_index)
    if key not in _TRAJ:
        _, m, P = want(case, b)
        _TRAJ[key] = (case, R.trajectories_fast(m, P, int(case[6][b]), n_traj, draw_index))      # (the case is kept alive: its id stays its own)
    return _TRAJ[key][1]
