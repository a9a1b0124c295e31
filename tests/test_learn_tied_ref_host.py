"""tests/learn_tied_ref.py's TiedLearner against exact arithmetic on one tiny case: three streams in two groups, k = 2.  Beside the
float learner run per-member learn_ref.Learner objects in Fractions under the same threshold words; the group's exact pooled record
is the sum of its members' exact records (no order matters there), and the tied table must be the M-step of that sum to rounding,
held by every member bit for bit, with the firing rule's events as the schedule sets them.  On the CPU."""
import math
from fractions import Fraction

import numpy as np

import learn_ref as G
import learn_tied_ref as T
import retable_ref as R

LOG_NORM = math.log(2 * 3.14159265358979323846 * 1.0 * 1.0)
GROUPS = [0, 1, 0]
SCHEDULE = [(2, 1, 1), (0, 3, 1), (3, 0, 1)]
T_MIN = 4


def test_the_tied_learner_is_the_m_step_of_the_exact_pooled_record():
    k, B = 2, 3
    rng = np.random.default_rng(5)
    gm, gt = rng.normal(0.0, 2.0, (2, k)), rng.uniform(0.1, 1.0, (2, k, k))
    means, trans = gm[GROUPS], gt[GROUPS]
    gamma = (np.arange(8) + 1.0) ** -0.6
    masses = [[[int(v) for v in rng.integers(1, 40, k)] for _ in range(5)] for _ in range(B)]
    obs = [rng.uniform(-3.0, 3.0, 5) for _ in range(B)]
    tied = T.TiedLearner(means, trans, k, GROUPS, gamma, T_MIN, LOG_NORM)
    exact = [G.Learner(means[b], trans[b], k, gamma, None, LOG_NORM, F=Fraction) for b in range(B)]
    lens = [0] * B
    for call, dT in enumerate(SCHEDULE):
        m_new = [masses[b][lens[b]:lens[b] + dT[b]] for b in range(B)]
        y_new = [obs[b][lens[b]:lens[b] + dT[b]] for b in range(B)]
        before = [(lr.means.copy(), lr.trans.copy(), lr.thr.copy(), lr.status) for lr in tied.learners]
        fired0 = list(tied.fired)
        for b in range(B):
            exact[b].thr = tied.learners[b].thr                 # (the words in force: the push reads its p from them)
            exact[b].advance(m_new[b], y_new[b])
        tied.advance(m_new, y_new)
        lens = [lens[b] + dT[b] for b in range(B)]
        for b in range(B):
            want = np.array([float(v) for v in exact[b].record])
            assert np.allclose(G.record_array(tied.learners[b].record), want, rtol=1e-12, atol=1e-15), "call %d, problem %d: the member's record" % (call, b)
        for g, mem in enumerate(tied.members):
            pooled = [sum((exact[b].record[e] for b in mem), Fraction(0)) for e in range(G.RECORD)]
            assert np.allclose(tied.pooled[g], [float(v) for v in pooled], rtol=1e-12, atol=1e-15), "call %d, group %d: the pooled record" % (call, g)
            fires = any(dT[b] for b in mem) and sum(lens[b] for b in mem) >= T_MIN
            assert tied.fired[g] - fired0[g] == int(fires)
            lead = tied.learners[mem[0]]
            for b in mem:
                lr = tied.learners[b]
                if not fires:
                    assert np.array_equal(lr.means, before[b][0]) and np.array_equal(lr.trans, before[b][1]) and np.array_equal(lr.thr, before[b][2]) and lr.status == before[b][3]
                    continue
                assert lr.status == 0
                assert np.array_equal(lr.means.view(np.uint64), lead.means.view(np.uint64)) and np.array_equal(lr.trans.view(np.uint64), lead.trans.view(np.uint64))
                assert np.array_equal(lr.thr, R.thresholds(lead.trans, k))
            if fires:
                for s in range(k):
                    row = sum(pooled[8 * s:8 * s + k], Fraction(0))
                    assert np.allclose(lead.trans[s], [float(pooled[8 * s + j] / row) for j in range(k)], rtol=1e-12)
                    assert math.isclose(lead.means[s], float(pooled[72 + s] / pooled[64 + s]), rel_tol=1e-11, abs_tol=1e-13)
    # group 0 = {0, 2} first fires in the second call, where its members' lengths 2 + 2 reach the burn-in no member has reached alone and
    # only problem 2 receives an observe; group 1 = {1} fires in the second call and is not fed in the third
    assert tied.fired == [2, 1] and lens == [5, 4, 3]
    # streams weigh equally: the pooled occupancy of a group is its number of members that hold an observe
    assert math.isclose(tied.pooled[0][64:64 + k].sum(), 2.0, rel_tol=1e-12) and math.isclose(tied.pooled[1][64:64 + k].sum(), 1.0, rel_tol=1e-12)
