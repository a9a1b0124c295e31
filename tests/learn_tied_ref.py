"""Tied online EM (csrc/batch_learn_tied.hpp, include/cpprob_hip.h: cpprob_hip_batch_learn_tie) restated in plain Python.  Nothing here
is new but the firing rule: the members are tests/learn_ref.py's Learner (or tests/scale_ref.py's ScaledLearner) with no M-step of
their own -- push and read only --, the pooled record is tests/pool_ref.py's compact sum, and the M-step, the check and the threshold
words are tests/retable_ref.py's (tests/scale_ref.py's on a scaled learner).  The reference of tests/test_learn_tied_ref_host.py,
tests/test_batch_learn_tied_kernel_text_host.py and tests/test_gpu_batch_learn_tied.py."""
import numpy as np

import learn_ref as G
import pool_ref as P
import retable_ref as R
import scale_ref as S


class TiedLearner:
    """The streams of a tied learning batch.  means [B, k], trans [B, k, k] (equal within a group), groups int [B], gamma the step
    sizes, t_min the observes a GROUP must have seen before its first M-step.  sigmas [B, k]: a scaled learner; floor None keeps the
    sigmas (a plain arming of a scaled batch).  State: learners (one a problem: means, trans, thr, tau, record, status, done and, scaled,
    sigmas and log_norms), pooled [G, 88]; fired[g]: the advances in which group g ran its M-step, changed[g]: those that replaced
    its table."""

    def __init__(self, means, trans, k, groups, gamma, t_min, log_norm=None, sigmas=None, floor=None, F=float):
        self.k, self.t_min, self.floor, self.scaled = k, int(t_min), floor, sigmas is not None
        self.groups = [int(g) for g in groups]
        self.members = P.members(self.groups)
        B = len(self.groups)
        if self.scaled:
            self.learners = [S.ScaledLearner(means[b], trans[b], sigmas[b], k, gamma, None, floor) for b in range(B)]
        else:
            self.learners = [G.Learner(means[b], trans[b], k, gamma, None, log_norm, F) for b in range(B)]
        self.pooled = np.zeros((len(self.members), G.RECORD))
        self.fired = [0] * len(self.members)
        self.changed = [0] * len(self.members)

    def advance(self, m_new, y_new):
        """m_new[b], y_new[b]: problem b's new m-table rows and observes (possibly none).  Every member's push and record under the
        words in force, the groups' pooled records, then one M-step a firing group from the table of its first member."""
        L = self.learners
        for b, lr in enumerate(L):
            lr.advance(m_new[b], y_new[b])                       # (t_min None: push and read only)
        rec = np.stack([G.record_array(lr.record) for lr in L])
        self.pooled = P.pool(rec, self.groups, broadcast=False)
        for g, mem in enumerate(self.members):
            fed = any(len(m_new[b]) > 0 for b in mem)
            seen = sum(int(L[b].done) for b in mem)
            if not fed or seen < self.t_min:
                continue
            self.fired[g] += 1
            lead = L[mem[0]]
            if self.scaled and self.floor is not None:
                means, sigmas, log_norms, trans = S.m_step(self.pooled[g], lead.means, lead.sigmas, lead.log_norms, lead.trans, self.k, self.floor)
            else:
                means, trans = R.m_step(self.pooled[g], lead.means, lead.trans, self.k)
                sigmas, log_norms = (lead.sigmas, lead.log_norms) if self.scaled else (None, None)
            bits = S.check(means, sigmas, trans, self.k) if self.scaled else R.check(means, trans, self.k)
            if bits == 0:
                self.changed[g] += 0 if (np.array_equal(means, lead.means) and np.array_equal(trans, lead.trans)) else 1
                thr = R.thresholds(trans, self.k)
            for b in mem:
                L[b].status = bits
                if bits == 0:
                    L[b].means, L[b].trans, L[b].thr = means.copy(), trans.copy(), thr.copy()
                    if self.scaled:
                        L[b].sigmas, L[b].log_norms = sigmas.copy(), log_norms.copy()

    def tables(self):
        L = self.learners
        return np.stack([lr.means for lr in L]), np.stack([lr.trans for lr in L])

    def status(self):
        return np.array([lr.status for lr in self.learners], np.int32)

    def records(self):
        return np.stack([G.record_array(lr.record) for lr in self.learners])
