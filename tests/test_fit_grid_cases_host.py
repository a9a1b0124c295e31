"""tests/fit_grid_cases.py reaches what it claims, proved on the CPU with tests/scale_ref.py and tests/retable_ref.py, so that the GPU
tests built on it (tests/test_gpu_batch_fit_domain.py, tests/test_gpu_batch_fit_grids.py) cannot pass vacuously.  No GPU."""
import math

import numpy as np

import fit_grid_cases as F
import retable_ref as R
import scale_ref as S
from test_scale_ref_host import ARGS


def test_log_sigmas_span_table_logs_domain():
    sg = F.log_sigmas()
    n = F.n_log_sigmas()
    assert len(ARGS) == 16043 and n >= 16000
    assert sg.shape == (2006, 8) and sg.size - n == 7 and np.all(sg.reshape(-1)[n:n + 4] == 1.0)
    assert not any(S.bad(s) for s in sg.reshape(-1))
    args = np.array([S.norm_arg(s) for s in sg.reshape(-1)])
    args = np.concatenate([args[:n], args[n + 4:]])                        # (the arguments from ARGS and the padding's BELOW_THE_FOLD)
    assert np.all(args >= S.MIN_NORMAL) and np.all(np.isfinite(args))
    exps = {math.frexp(a)[1] for a in args}
    m = np.array([math.frexp(a)[0] * 2.0 for a in args])                  # the mantissa in [1, 2) table_log folds at sqrt(2)
    below = int(np.sum((m < S.SQRT2) & (m >= S.SQRT2 - 1e-3)))
    above = int(np.sum((m >= S.SQRT2) & (m <= S.SQRT2 + 1e-3)))
    near_one = int(np.sum(np.abs(args - 1.0) <= 1e-3))
    print("log_sigmas: %d survivors of %d, %d distinct exponents %d .. %d, %d + %d mantissas within 1e-3 below / above the fold, %d arguments within 1e-3 of 1"
          % (n, len(ARGS), len(exps), min(exps), max(exps), below, above, near_one))
    assert len(exps) >= 1900
    assert below >= 10 and above >= 10
    assert near_one >= 1000


def test_fused_case_shows_a_contracted_table_log():
    """Every sigma of fused_case has a log_norm that changes where table_log's products and sums are fused; none of log_sigmas() has."""
    v, sg = F.fused_case()
    assert v.shape == sg.shape == (8, 8) and not any(S.bad(s) for s in sg.reshape(-1))
    assert np.array_equal(sg, [[math.sqrt(x) for x in row] for row in v])
    args = [S.norm_arg(s) for s in sg.reshape(-1)]
    assert len({math.frexp(a)[1] for a in args}) >= 6
    for i, a in enumerate(args):
        assert F.table_log_fused(a, False, False, False) == S.table_log(a)
        assert F.table_log_fused(a) != S.table_log(a), i
        assert (F.table_log_fused(a, horner=False, lo=False) != S.table_log(a)) == (i >= 1), i
        assert (F.table_log_fused(a, q=False, lo=False) != S.table_log(a)) == (i <= 1), i
        assert F.table_log_fused(a, horner=False, q=False) == S.table_log(a), i
    # through the M-step: occ = 1 and occ_yy = v give back the sigma
    assert all(S.sigma_step(1.0, x, 0.0, F.SIGMA_FLOOR) == s for x, s in zip(v.reshape(-1), sg.reshape(-1)))
    hidden = [s for s in F.log_sigmas().reshape(-1) if F.table_log_fused(S.norm_arg(s)) != S.log_norm(s)]
    print("fused_case: 64 arguments over %d binary exponents; of log_sigmas() a fused table_log changes %d" % (len({math.frexp(a)[1] for a in args}), len(hidden)))
    assert len(hidden) <= 2                                               # (which is why fused_case exists)


def test_division_case_shows_a_quotient_one_ulp_off():
    y, means, sigmas = F.division_case()
    B = F.log_sigmas().shape[0]
    assert y.shape == (B,) and means.shape == sigmas.shape == (B, 8) and B * 8 >= 16000
    d = y[:, None] - means
    assert np.array_equal((d + means), np.broadcast_to(y[:, None], d.shape)) and np.array_equal(d, np.broadcast_to(y[:, None], d.shape))
    es = np.frexp(sigmas)[1] - 1
    assert es.min() == -20 and es.max() == 20
    q = d / sigmas
    assert np.all(np.abs(q) >= 2.0 ** 10) and np.all(np.abs(q) < 2.0 ** 60)
    eq = np.frexp(q)[1] - 1
    assert eq.min() == 10 and eq.max() == 59 and np.any(q < 0.0) and np.any(q > 0.0)
    ln = np.array([[S.log_norm(s) for s in row] for row in sigmas])
    want = np.stack([S.rows(y[b:b + 1], means[b], sigmas[b], 8)[0] for b in range(B)])
    row = F.row_from_quotient(q, ln)
    assert np.array_equal(row.view(np.uint64), want.view(np.uint64))      # (row_from_quotient is scale_ref.rows behind its division)
    for side in (-np.inf, np.inf):
        moved = F.row_from_quotient(np.nextafter(q, side), ln)
        share = float(np.mean(moved.view(np.uint64) != row.view(np.uint64)))
        print("division_case: a quotient one ulp towards %s changes %.2f %% of %d entries" % (side, 100.0 * share, q.size))
        assert share >= 0.99


def test_mstep_records_take_every_branch():
    rec, means, trans, sigmas = F.mstep_records()
    B = F.log_sigmas().shape[0]
    assert rec.shape == (B, R.RECORD) and np.all(rec[:, 72:80] == 0.0)
    occ = rec[:, 64:72]
    live = occ > 0.0
    assert np.all((occ[live] >= 1.0) & (occ[live] < 2.0))
    floor = F.SIGMA_FLOOR
    root = floored = refused = massless = 0
    exps = set()
    for b in range(B):
        m, sg, ln, tr = S.m_step(rec[b], means[b], sigmas[b], np.full(8, -7.0), trans[b], 8, floor)
        for s in range(8):
            if not occ[b, s] > 0.0:
                massless += 1
                assert sg[s] == sigmas[b, s] and ln[s] == -7.0 and m[s] == means[b, s]
                continue
            assert m[s] == 0.0
            v = rec[b, 80 + s] / occ[b, s]
            if v >= floor * floor:
                root += 1
                assert sg[s] == math.sqrt(v)
                exps.add(math.frexp(sg[s])[1])
            else:
                floored += 1
                assert sg[s] == floor
            if math.isnan(ln[s]):
                refused += 1
                assert S.bad(sg[s])
        if b % 7 == 0:
            assert np.array_equal(tr[1], trans[b, 1]) and not np.array_equal(tr[0], trans[b, 0])
    print("mstep_records: %d states: %d take the square root (%d binary exponents), %d the floor, %d refused, %d without mass"
          % (B * 8, root, len(exps), floored, refused, massless))
    assert root >= 0.95 * B * 8 and B * 8 - refused - massless >= 0.95 * B * 8
    assert floored >= 1 and refused >= 1 and massless >= 1 and len(exps) >= 900
    # the square roots run over log_sigmas(): each within a few ulps of the sigma it was built from
    want = F.log_sigmas().reshape(-1)[:F.n_log_sigmas()]
    got = np.sqrt(rec[:, 80:88].reshape(-1)[:want.size] / occ.reshape(-1)[:want.size])
    normal = want * want >= S.MIN_NORMAL * 4.0
    assert np.all(np.abs(got[normal] - want[normal]) <= 4.0 * np.spacing(want[normal]))


def test_many_problems_make_a_workgroup_walk_two_tiles():
    assert R.grid_y(70, 1366) == 2 and F.tiles_walked(70, 1366) == [[0, 2], [1]]
    assert R.grid_y(70, 1365) == 3 and F.tiles_walked(70, 1365) == [[0], [1], [2]]
    assert R.grid_y(33, 2049) == 1 and F.tiles_walked(33, 2049) == [[0, 1]]
    Ts, obs, A, Bt = F.many_problems(1366)
    assert len(Ts) == 1366 and set(Ts) == set(F.LENGTHS) and Ts[-1] == 70 and [len(o) for o in obs] == Ts
    assert all(a.shape[0] == 1366 for a in A + Bt) and not np.array_equal(A[0], Bt[0]) and not np.array_equal(A[2], Bt[2])
    # the learn-rows kernels share the grid: the second advance's longest piece is 70 and starts at an unaligned row
    first, second = F.learn_schedule(1366)
    assert set(first) == {F.LEARN_FIRST} and F.LEARN_FIRST % R.ROWS_PER_TRIP != 0 and {0, 31, 32, 33, 65, 70} <= set(second)
    assert max(second) == 70 and R.grid_y(max(second), 1366) == 2 and all(a + b <= F.LEARN_CAP for a, b in zip(first, second))
