"""The tolerance of tests/test_gpu_batch_mix.py::test_exact_fit_is_baum_welch, measured without a GPU: the largest distance, over
exactly that test's case, between the restatement chain the device equals bit for bit (tests/mix_ref.py's rows, tests/exact_ref.py's
run, tests/suffstats_ref.py's record on coordinate 0, mix_ref's sums and M-step) and the test's float64 Baum-Welch.  It also checks
that the float64 reference neither swaps nor kills a component within the test's five iterations.
Run from the repository root: python tools/measure_mix_tolerance.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import backward_ref as R  # noqa: E402
import exact_ref as X  # noqa: E402
import mix_ref as MR  # noqa: E402
import suffstats_ref as SS  # noqa: E402
import test_gpu_batch_mix as T  # noqa: E402


def chain(obs, W, Mu, Sg, A, iterations, floor=1e-6):
    k = Mu.shape[0]
    hist = [(W.copy(), Mu.copy(), Sg.copy(), A.copy())]
    for _ in range(iterations):
        P = R.transition_masses(A)
        m, _, dead = X.run(MR.rows(obs, W, Mu, Sg)[:, :k].tolist(), P)
        assert dead == -1
        rec = np.concatenate([SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[:, 0])), MR.sums(m, P, obs, W, Mu, Sg)])
        W, Mu, Sg, A = MR.m_step(rec, W, Mu, Sg, A, floor)
        hist.append((W.copy(), Mu.copy(), Sg.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


if __name__ == "__main__":
    worst = 0.0
    obs, W, Mu, Sg, A = T.two_mode_case()
    for b in range(2):
        got, want = chain(obs[b], W[b], Mu[b], Sg[b], A[b], 5), T.baum_welch(obs[b], W[b], Mu[b], Sg[b], A[b], 5)
        # (no swap: every component stays the nearest to its own starting mean; no kill: every weight stays above 0.2)
        near = np.linalg.norm(want[1][:, :, :, None, :] - Mu[b][None, :, None, :, :], axis=-1).argmin(axis=-1)
        assert (near == np.arange(2)[None, None, :]).all() and want[0].min() > 0.2, "the float64 reference swaps or kills a component"
        dist = [np.abs(g[1:] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: weights %.3g, means %.3g, sigmas %.3g, transition rows %.3g; smallest weight %.3f" % (b, *dist, want[0].min()))
        worst = max(worst, *dist)
    print("largest distance %.3g; the test's tolerance is eight times it" % worst)
