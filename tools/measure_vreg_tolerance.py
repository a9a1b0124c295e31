"""The tolerance of tests/test_gpu_batch_vreg.py::test_exact_fit_is_baum_welch, measured without a GPU: the largest distance, over exactly
that test's case, between the restatement chain the device equals bit for bit (tests/vreg_ref.py's exact_em: its rows, tests/exact_ref.py's
run, tests/suffstats_ref.py's record on coordinate 0, full_ref's sums, vreg_ref's M-step) and the test's float64 Baum-Welch.  It also
asserts what makes eight times that base mean what it says: the reference EM's evidence never decreases, every state keeps mass in every
iteration, and no state changes places (the final coefficients are nearest their own start).
Run from the repository root: python tools/measure_vreg_tolerance.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import test_gpu_batch_vreg as T  # noqa: E402
import vreg_ref as VR  # noqa: E402

if __name__ == "__main__":
    worst = 0.0
    obs, C, V, A = T.switching_case()
    for b in range(2):
        (got, ev, low), want = VR.exact_em(obs[b], C[b], V[b], A[b], 5, 1e-3), T.baum_welch(obs[b], C[b], V[b], A[b], 5)
        assert (np.diff(ev) >= 0.0).all() and low > 1.0, (ev, low)
        for s in range(2):
            assert np.argmin([np.abs(want[0][-1][s] - C[b][j]).sum() for j in range(2)]) == s
        dist = [np.abs(g[1:] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: coefficients %.3g, covariances %.3g, transition rows %.3g; log-evidences %s; smallest occupancy %.3g" % (b, *dist, np.round(ev, 4), low))
        worst = max(worst, *dist)
    print("largest distance %.3g; the test's tolerance is eight times it" % worst)
