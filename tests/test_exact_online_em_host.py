"""How far the exact stream's learner stands from float64 (no GPU): the restatement the device equals -- tests/exact_ref.py's rows pushed
through tests/learn_ref.py with gamma[t] = 1 / (t + 1) -- against a forward-only smoother in numpy float64, k = 2, T = 64.  What
separates them is rounding (the 2^-32 grids of the transition masses and the weights, the 2^-44 grid of m), not sampling."""
import numpy as np

import backward_ref as R
import exact_ref as X
import learn_ref as G

MEANS, TRANS, T = np.array([-1.0, 1.5]), np.array([[0.9, 0.1], [0.3, 0.7]]), 64
# the largest difference of the final records' 88 entries, measured with this file (profiles/r39_notes.md); the bound is 4 times it
MEASURED, FACTOR = 5.41e-11, 4.0


def float_record(y, means, trans, gamma):
    k = len(means)
    tau, phi = np.zeros((k, G.RECORD)), None
    for t, yt in enumerate(y):
        g, lik, new = gamma[t], np.exp(-0.5 * (yt - means) ** 2), np.zeros((k, G.RECORD))
        if t > 0:
            a = phi[:, None] * trans
            for sn in range(k):
                v = (1.0 - g) * tau
                v[np.arange(k), 8 * np.arange(k) + sn] += g
                new[sn] = (a[:, sn] / a[:, sn].sum()) @ v
        for sn in range(k):
            new[sn, [64 + sn, 72 + sn, 80 + sn]] += [g, g * yt, g * yt * yt]
        phi = lik / k if t == 0 else a.sum(0) * lik
        tau, phi = new, phi / phi.sum()
    return phi @ tau


def test_the_exact_learners_record_is_float64s_within_rounding():
    rng = np.random.default_rng(39)
    x = [0]
    for _ in range(T - 1):
        x.append(int(rng.random() >= TRANS[x[-1], 0]))
    y = MEANS[x] + rng.standard_normal(T)
    gamma = 1.0 / (np.arange(T) + 1.0)
    m = X.run(np.array(R.log_likelihoods(y, MEANS)).tolist(), R.transition_masses(TRANS))[0]
    lr = G.Learner(MEANS, TRANS, 2, gamma, None, 0.0)
    lr.advance([[int(v) for v in row[:2]] for row in m], y)
    diff = np.abs(G.record_array(lr.record) - float_record(y, MEANS, TRANS, gamma)).max()
    print("largest difference of the final record: %.3g" % diff)
    assert 0.0 < diff <= FACTOR * MEASURED
