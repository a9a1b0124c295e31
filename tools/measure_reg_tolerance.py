"""The tolerance of tests/test_gpu_batch_reg.py::test_exact_fit_is_baum_welch, measured without a GPU: the largest distance, over
exactly that test's case, between the restatement chain the device equals bit for bit (tests/reg_ref.py's rows, tests/exact_ref.py's
run, tests/suffstats_ref.py's record on coordinate 0, full_ref's sums, reg_ref's M-step) and the test's float64 Baum-Welch.  It also
asserts that the reference keeps each state nearest its own starting coefficients and that no smoothed posterior of the chain's first
run is within 1e-6 of 0 or 1 (the run's quantum is 2^-44) -- well-separated regimes would hide the run's quantisations -- and prints the
share of steps whose marginals lie in [0.1, 0.9].
Run from the repository root: python tools/measure_reg_tolerance.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import backward_ref as R  # noqa: E402
import exact_ref as X  # noqa: E402
import full_ref as FR  # noqa: E402
import reg_ref as RR  # noqa: E402
import suffstats_ref as SS  # noqa: E402
import test_gpu_batch_reg as T  # noqa: E402


def chain(obs, C, Sg, A, iterations, floor=1e-3):
    k, P = C.shape
    hist, spread = [(C.copy(), Sg.copy(), A.copy())], None
    for _ in range(iterations):
        Pm = R.transition_masses(A)
        m, _, dead = X.run(RR.rows(obs, C, Sg)[:, :k].tolist(), Pm)
        assert dead == -1
        mr = [[int(v) for v in row[:k]] for row in m]
        if spread is None:
            g = np.asarray(R.marginals(mr, Pm), np.float64)
            spread = (g.min(), g.max(), np.mean((g[:, 0] >= 0.1) & (g[:, 0] <= 0.9)))
        rec = np.concatenate([SS.record(SS.stats(mr, Pm, obs[:, 0])), FR.sums(m, Pm, obs, 1 + P)])
        C, Sg, _, A = RR.m_step(rec, C, Sg, A, floor)
        hist.append((C.copy(), Sg.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)], spread


if __name__ == "__main__":
    worst = 0.0
    obs, C, Sg, A = T.switching_case()
    for b in range(2):
        (got, spread), want = chain(obs[b], C[b], Sg[b], A[b], 5), T.baum_welch(obs[b], C[b], Sg[b], A[b], 5)
        for s in range(2):                                  # (no label switch: the final coefficients are nearest their own start)
            assert np.argmin([np.abs(want[0][-1][s] - C[b][j]).sum() for j in range(2)]) == s
        assert 1e-6 < spread[0] and spread[1] < 1 - 1e-6, spread
        dist = [np.abs(g[1:] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: coefficients %.3g, sigmas %.3g, transition rows %.3g; first run's marginals in [%.3g, %.6g], %.0f%% of the steps in [0.1, 0.9]" % (b, *dist, *spread[:2], 100 * spread[2]))
        worst = max(worst, *dist)
    print("largest distance %.3g; the test's tolerance is eight times it" % worst)
