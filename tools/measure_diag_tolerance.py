"""The tolerance of tests/test_gpu_batch_diag.py::test_exact_fit_is_baum_welch, measured without a GPU: the largest distance, over
exactly that test's cases, between the restatement chain the device equals bit for bit (tests/diag_ref.py's rows, tests/exact_ref.py's
run, tests/suffstats_ref.py's record on coordinate 0, diag_ref's sums and M-step) and the test's float64 Baum-Welch.
Run from the repository root: python tools/measure_diag_tolerance.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import backward_ref as R  # noqa: E402
import diag_ref as DR  # noqa: E402
import exact_ref as X  # noqa: E402
import suffstats_ref as SS  # noqa: E402
import test_gpu_batch_diag as T  # noqa: E402


def chain(obs, M, Sg, A, iterations, floor=1e-3):
    k, D = M.shape
    hist = [(M.copy(), Sg.copy(), A.copy())]
    for _ in range(iterations):
        P = R.transition_masses(A)
        m, _, dead = X.run(DR.rows(obs, M, Sg)[:, :k].tolist(), P)
        assert dead == -1
        sy, syy = DR.sums(m, P, obs, D)
        rec = np.concatenate([SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[:, 0])), np.stack([sy, syy], axis=1).reshape(-1)])
        M, Sg, A = DR.m_step(rec, M, Sg, A, floor)
        hist.append((M.copy(), Sg.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


if __name__ == "__main__":
    worst = 0.0
    c = T._case(2, 3, (37, 37), seed=6)
    for b in range(2):
        got, want = chain(c["obs"][b], c["M"][b], c["S"][b], c["A"][b], 5), T.baum_welch(c["obs"][b], c["M"][b], c["S"][b], c["A"][b], 5)
        dist = [np.abs(g[1:] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: means %.3g, sigmas %.3g, transition rows %.3g" % (b, *dist))
        worst = max(worst, *dist)
    print("largest distance %.3g; the test's tolerance is eight times it" % worst)
