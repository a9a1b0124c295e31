"""The tolerance of tests/test_gpu_batch_categorical.py::test_exact_fit_is_baum_welch, measured without a GPU: the largest distance,
over exactly that test's cases, between the restatement chain the device equals bit for bit (tests/categorical_ref.py's rows,
tests/exact_ref.py's run, tests/suffstats_ref.py's record, categorical_ref's counts and M-step) and the test's float64 Baum-Welch.
Run from the repository root: python tools/measure_categorical_tolerance.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import backward_ref as R  # noqa: E402
import categorical_ref as CR  # noqa: E402
import exact_ref as X  # noqa: E402
import suffstats_ref as SS  # noqa: E402
import test_gpu_batch_categorical as T  # noqa: E402


def chain(obs, E, A, iterations, floor=1e-6):
    k, V = E.shape
    Es, As = [E.copy()], [A.copy()]
    for _ in range(iterations):
        P = R.transition_masses(A)
        m, _, dead = X.run(CR.rows(obs, E)[:, :k].tolist(), P)
        assert dead == -1
        rec = np.concatenate([SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs)), CR.symbol_counts(m, P, obs, V).reshape(-1)])
        E, A = CR.m_step(rec, E, A, floor)
        Es.append(E.copy())
        As.append(A.copy())
    return np.array(Es), np.array(As)


if __name__ == "__main__":
    worst = 0.0
    for k, V in ((2, 4), (3, 9)):
        c = T._case(k, V, (37, 37), seed=5)
        for b in range(2):
            got, want = chain(c["obs"][b], c["E"][b], c["A"][b], 5), T.baum_welch(c["obs"][b], c["E"][b], c["A"][b], 5)
            dE, dA = np.abs(got[0] - want[0]).max(), np.abs(got[1][1:] - want[1][1:]).max()
            print("k %d V %d problem %d: matrix %.3g, transition rows %.3g" % (k, V, b, dE, dA))
            worst = max(worst, dE, dA)
    print("largest distance %.3g; the test's tolerance is eight times it" % worst)
