"""The cases of tests/csmc_grid_cases.py and the statistics shapes of tests/test_gpu_batch_trajstats_grid.py proven without a GPU: the
cases' own preconditions hold on the plain references, and the cases go through the sanitized stand-alone programs of
tests/test_batch_csmc_kernel_text_host.py and tests/test_batch_trajstats_kernel_text_host.py (the kernels' own text as host code,
every buffer of exactly the size the host code hands the kernel).  Nothing is loaded into python and nothing runs on a GPU."""
import numpy as np
import pytest

import backward_ref as R
import csmc_grid_cases as G
import csmc_ref as CS
import test_batch_csmc_kernel_text_host as CK
import test_batch_trajstats_kernel_text_host as TK
import trajstats_ref as TS
from test_batch_csmc_kernel_text_host import prog as csmc_prog  # noqa: F401  (the module-scoped fixtures that build the programs,
from test_batch_trajstats_kernel_text_host import prog as stats_prog  # noqa: F401   under the names this file asks for them by)

TILE = TK.TILE


def _batch(case):
    """The case as the kernel-text program's batch: its tables' thresholds, its log-likelihood rows, its reference bytes."""
    k, Ts, ns, means, trans, obs, seeds, paths = case
    described = len(means) > 1
    rows = [R.thresholds(tr) for tr in trans]
    ll = [R.log_likelihoods(obs[b], G.table(case, b)[0]) for b in range(len(Ts))]
    return CK.Batch.given(Ts, ns, k, described, seeds, rows, ll, paths)


def _check(prog, case, what):
    bt = _batch(case)
    if bt.described:
        assert bt.order == G.dispatch_order(case[1], case[2])
    want = bt.want()
    for b in range(bt.B):                                        # (Batch.want and the cases' want are one reference)
        assert np.array_equal(want[b, :bt.Ts[b]], G.want(case, b)[0])
    got = prog(bt)
    bad = sorted({int(b) for b in np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:, 0]})
    assert not bad, "%s: rows differ from the reference in problems %s" % (what, bad)


# ---- the cases' own preconditions, on the references alone --------------------------------------------------------------------------
def test_long_case_visits_the_last_state_of_every_bank():
    """LONG's reference trajectories (TILE + 1 of them, draw_index 65535) visit state 7, and some record has xi[7][7], occ_y[7] and
    occ_yy[7] non-zero: the last counter and the last accumulators of batch_traj_stats_kernel<8> leave zero."""
    case = G.long_case()
    assert case[0] == 8 and case[4][1, 0, 7] == 0.0 and max(case[1]) == 1500 and max(case[2]) == 8192
    b = 2                                                        # (T = 63, n = 70: the whole case's trajectories belong to the GPU file)
    traj = G.trajectories(case, b, TILE + 1, G.LONG_DRAW)
    rec = TS.records(traj, case[5][b])
    assert np.any(traj == 7) and np.any(rec[:, 8 * 7 + 7] > 0) and np.any(rec[:, 72 + 7] != 0.0) and np.any(rec[:, 80 + 7] != 0.0)


def test_many_case_is_ragged_and_out_of_order():
    for reverse in (False, True):
        Ts, ns = G.many_lengths(G.MANY_B, reverse)
        order = G.dispatch_order(Ts, ns)
        assert len(Ts) == 300 and all(Ts[b] != Ts[b + 1] for b in range(299)) and ns[17] == 1025
        assert sum(1 for i, b in enumerate(order) if i != b) >= 290
    case = G.many_case()
    assert np.all(case[4][1::5, 0, 7] == 0.0) and np.all(case[4][0::5, 0, 7] > 0.0)
    assert G.many_case(reverse=True)[1] == case[1][::-1] and len(G.many_case(301)[1]) == 301


def test_one_hot_case_holds_its_edges():
    """Rows with one non-zero mass under several occupied states, occupied states of mass 0 (the case asserts both itself), and the
    n = 1 problem: rows one-hot at the reference path, and a backward trajectory that is that path -- where the table forbids the
    path's step (out of the absorbing state 1, or 0 -> 7) through the smoother's defensive rule."""
    case = G.one_hot_case()
    k, Ts, ns, means, trans, obs, seeds, paths = case
    xs, m = G.states(case, 2)
    occupied = np.array([np.bincount(x, minlength=k) > 0 for x in xs])
    nonzero = np.array(m) > 0
    lone, starved = int(np.sum((nonzero.sum(axis=1) == 1) & (occupied.sum(axis=1) > 1))), int(np.sum(occupied & ~nonzero))
    print("n = 300: %d rows of %d with one non-zero mass under several occupied states, %d occupied states of mass 0" % (lone, Ts[2], starved))
    assert lone >= 1 and starved >= 1
    rows, m1, P = G.want(case, 0)
    assert ns[0] == 1 and np.array_equal(np.nonzero(rows)[1], paths[0]) and np.all((rows > 0).sum(axis=1) == 1)
    assert any(P[int(paths[0][t])][int(paths[0][t + 1])] == 0 for t in range(Ts[0] - 1)), "the reference path should take a step its table forbids"
    assert np.array_equal(R.trajectories(m1, P, int(seeds[0]), 1)[:, 0], paths[0])


def test_bytes_cases_cover_the_documented_tolerance():
    for k in (5, 2):
        case = G.bytes_case(k)
        flat = np.concatenate(case[7]).astype(np.int64)
        assert flat.min() < 0 and np.any((flat & 7) >= k)
        for b in range(3):                                       # the reference on the bytes is the reference on the states they stand for
            clean = np.minimum(case[7][b].astype(np.int64) & 7, k - 1)
            means, tr = G.table(case, b)
            assert G.want(case, b)[1] == CS.masses(R.log_likelihoods(case[5][b], means), R.thresholds(tr), int(case[6][b]), case[2][b], clean)


# ---- the cases through the kernel's text ----------------------------------------------------------------------------------------------
def test_long_case_cut_short_through_the_kernel_text(csmc_prog):
    """LONG with its two longest problems at 129 steps (512 steps stay): every n of the case, k = 8, the zero entry."""
    case = G.long_case_cut(129)
    assert sorted(case[1]) == [1, 2, 63, 64, 65, 129, 129, 129, 512]
    _check(csmc_prog, case, "LONG, cut")


def test_one_hot_case_through_the_kernel_text(csmc_prog):
    _check(csmc_prog, G.one_hot_case(), "ONE_HOT")


@pytest.mark.parametrize("k", [5, 2])
def test_bytes_case_through_the_kernel_text(csmc_prog, k):
    _check(csmc_prog, G.bytes_case(k), "BYTES, k = %d" % k)


@pytest.mark.parametrize("k", [2, 8])
def test_statistics_shapes_through_the_kernel_text(stats_prog, k):
    """T = 512 staged in LDS and T = 513 read from memory, n_traj = 2 TILE + 5 (three tiles, the last partial), the largest
    draw_index; at k = 8 state 7 is visited, so the last register of each bank and the rows 7 of the mapping carry numbers."""
    bt = TK.Batch(G.STATS_TS, G.STATS_NS, k, False, 300 + k)
    n_traj = 2 * TILE + 5
    want = bt.want(n_traj, draw_index=65535)
    if k == 8:
        assert np.any(want[:, :, 8 * 7 + 7] > 0) and np.any(want[:, :, 8 * 7 + 6] != want[:, :, 8 * 6 + 7])
        assert np.any(want[:, :, 72 + 7] != 0.0) and np.any(want[:, :, 80 + 7] != 0.0)
    got = stats_prog(bt, n_traj, draw_index=65535)
    assert np.array_equal(got, want), "k = %d: records differ from the reference in problems %s" % (k, sorted({int(b) for b in np.argwhere(got != want)[:, 0]}))
