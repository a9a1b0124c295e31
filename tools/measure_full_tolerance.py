"""The tolerance of tests/test_gpu_batch_full.py::test_exact_fit_is_baum_welch, measured without a GPU: the largest distance, over
exactly that test's case, between the restatement chain the device equals bit for bit (tests/full_ref.py's rows, tests/exact_ref.py's
run, tests/suffstats_ref.py's record on coordinate 0, full_ref's sums and M-step) and the test's float64 Baum-Welch.
Run from the repository root: python tools/measure_full_tolerance.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import backward_ref as R  # noqa: E402
import exact_ref as X  # noqa: E402
import full_ref as FR  # noqa: E402
import suffstats_ref as SS  # noqa: E402
import test_gpu_batch_full as T  # noqa: E402


def chain(obs, M, C, A, iterations, floor=1e-6):
    k, D = M.shape
    hist = [(M.copy(), C.copy(), A.copy())]
    for _ in range(iterations):
        P = R.transition_masses(A)
        m, _, dead = X.run(FR.rows(obs, M, C)[:, :k].tolist(), P)
        assert dead == -1
        rec = np.concatenate([SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[:, 0])), FR.sums(m, P, obs, D)])
        M, C, A = FR.m_step(rec, M, C, A, floor)
        hist.append((M.copy(), C.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


if __name__ == "__main__":
    worst = 0.0
    obs, M, C, A = T.correlated_case()
    for b in range(2):
        got, want = chain(obs[b], M[b], C[b], A[b], 5), T.baum_welch(obs[b], M[b], C[b], A[b], 5)
        dist = [np.abs(g[1:] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: means %.3g, covariances %.3g, transition rows %.3g" % (b, *dist))
        worst = max(worst, *dist)
    print("largest distance %.3g; the test's tolerance is eight times it" % worst)
