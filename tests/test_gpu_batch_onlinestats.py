"""Running sufficient statistics of an online batch (include/cpprob_hip.h: cpprob_hip_batch_online_stats, _online_stats_device,
_online_stats_progress; csrc/batch_onlinestats.hpp) against the plain-Python restatement of the forward-only recursion
(tests/onlinestats_ref.py), bit for bit.  The reference runs on the m table the device holds: cpprob_hip_batch_copy_masses' rows for a
keep_masses batch, backward_ref.filtering_masses of the rows of cpprob_hip_batch_copy_store for a batch with history.

The long walk is compared with cpprob_hip_batch_smooth_stats of the same batch as well: r = |forward - backward| / max(1, |backward|)
in units of T 2^-52 stays below 4 times the worst the two CPU references show on the cases of tests/test_onlinestats_ref_host.py
(0.62; that file states the measurement)."""
import ctypes as C

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import onlinestats_ref as N
from oracle import exact

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
R_BOUND = 4 * 0.62                              # tests/test_onlinestats_ref_host.py: R_WORST


def _seeds(nb, base=77):
    return np.array([base + 7919 * b for b in range(nb)], np.uint64)


def _tables(k, nb, seed):
    """Table 1 has a zero transition entry."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (nb, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (nb, k, k))
    if nb > 1:
        trans[1, 0, k - 1] = 0.0
    return means, trans


def _table_observes(means, Ts, seed):
    rng = np.random.default_rng(seed)
    k = means.shape[1]
    return [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]


def _record(stats, b):
    return np.concatenate([stats["xi"][b].reshape(-1), stats["occ"][b], stats["occ_y"][b], stats["occ_yy"][b]])


class Stream:
    """An online batch on `engine` and, a problem, the reference's running state.  masses: keep_history=False, keep_masses=True."""

    def __init__(self, engine, model, caps, ns, obs, tables=None, masses=False, seeds=None, with_obs=True):
        self.eng, self.model, self.obs, self.masses, self.with_obs = engine, model, obs, masses, with_obs
        self.B = len(caps)
        if model == cp.MODEL_HMM3:
            self.k, self.means, trans = 3, [exact.HMM_MEAN] * self.B, [exact.HMM_T] * self.B
        else:
            self.k, self.means, trans = tables[0].shape[1], tables[0], tables[1]
        self.P = [R.transition_masses(trans[b]) for b in range(self.B)]
        self.lens = [0] * self.B
        self.runs = [N.Running() for _ in range(self.B)]
        engine.batch_begin_online(model, caps, ns, _seeds(self.B) if seeds is None else seeds, tables=tables, keep_history=not masses, keep_masses=masses)

    def advance(self, dT):
        piece = [self.obs[b][self.lens[b]:self.lens[b] + dT[b]] for b in range(self.B)]
        self.eng.batch_advance(piece)
        self.lens = [self.lens[b] + dT[b] for b in range(self.B)]
        return piece

    def table(self, b):
        """Problem b's rows of the m table at the length reached, as integers."""
        L = self.lens[b]
        if L == 0:
            return []
        if self.masses:
            rows = self.eng.batch_masses(b)
            assert rows.shape == (L, 8) and np.all(rows[:, self.k:] == 0.0)
            return N.int_masses(rows, self.k)
        vals = self.eng.batch_store(b)[0]
        return R.filtering_masses(vals, R.log_likelihoods(self.obs[b][:L], self.means[b]))

    def want(self):
        """The reference's records at the lengths reached (consumes the new steps)."""
        out = []
        for b in range(self.B):
            m = self.table(b)
            self.runs[b].consume(m, self.P[b], self.obs[b] if self.with_obs else None)
            out.append(N.as_array(self.runs[b].read(m)))
        return np.stack(out)

    def check(self, piece, what=""):
        """A statistics call that consumes `piece`, against the reference; returns the records [B, 88]."""
        stats = self.eng.batch_online_stats(piece if self.with_obs else None)
        got = np.stack([_record(stats, b) for b in range(self.B)])
        want = self.want()
        for b in range(self.B):
            assert np.array_equal(got[b], want[b]), "%sproblem %d at length %d: largest difference %.3g" % (what, b, self.lens[b], np.abs(got[b] - want[b]).max())
        assert np.array_equal(self.eng.batch_online_stats_progress(), np.array(self.lens, np.uint32)), what
        return got


# ---- 1. a ragged batch, both sources of the m table ------------------------------------------------------------------------------
RAGGED = [(1, 1, 3, 0, 3), (0, 1, 1, 3, 0), (0, 0, 3, 1, 3), (0, 0, 0, 3, 1), (0, 0, 0, 3, 3), (0, 0, 0, 1, 1), (0, 0, 0, 1, 1)]


@pytest.mark.parametrize("masses", [False, True], ids=["history", "masses"])
def test_ragged_table_batch_after_every_advance(engine, masses):
    caps, ns, k = [1, 2, 7, 12, 12], [1, 5, 64, 300, 300], 3
    means, trans = _tables(k, 5, 61)
    obs = _table_observes(means, caps, 61)
    st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans), masses)
    assert np.all(engine.batch_online_stats_progress() == 0)
    for a, dT in enumerate(RAGGED):
        got = st.check(st.advance(dT), "advance %d, " % a)
        for b in range(5):
            L = st.lens[b]
            if L == 0:
                assert np.all(got[b] == 0.0)
                continue
            # the record is a set of expected counts: visits sum to L, transitions to L - 1 (within rounding)
            assert abs(got[b, 64:72].sum() - L) <= 1e-9 and abs(got[b, :64].sum() - (L - 1)) <= 1e-9
            xi = got[b, :64].reshape(8, 8)
            assert np.all(xi[k:] == 0.0) and np.all(xi[:, k:] == 0.0) and np.all(got[b, 64:].reshape(3, 8)[:, k:] == 0.0)
    assert st.lens == caps
    assert st.P[1][0][k - 1] == 0, "table 1 should hold a zero transition mass"


# ---- 2. the bits do not depend on the cuts ---------------------------------------------------------------------------------------
def test_cuts_do_not_change_the_bits(engine):
    caps, ns, k = [9, 5, 12], [64, 3, 300], 3
    means, trans = _tables(k, 3, 71)
    obs = _table_observes(means, caps, 71)
    finals = []
    # one observe at a time with a call a step; uneven pieces with calls in between (and one advance without a call); whole, one call
    one = [tuple(1 if t < c else 0 for c in caps) for t in range(12)]
    uneven = [((4, 0, 1), True), ((0, 2, 6), False), ((3, 3, 0), True), ((2, 0, 5), True)]
    for name, schedule in (("steps", [(dT, True) for dT in one]), ("pieces", uneven), ("whole", [(tuple(caps), True)])):
        st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans))
        owed = [np.zeros(0)] * 3
        for dT, call in schedule:
            piece = st.advance(dT)
            owed = [np.concatenate([owed[b], piece[b]]) for b in range(3)]
            if call:
                got = st.check(owed, name + ": ")
                owed = [np.zeros(0)] * 3
        assert st.lens == caps
        finals.append(got)
    assert np.array_equal(finals[0], finals[1]) and np.array_equal(finals[0], finals[2])


# ---- 3. nothing new ---------------------------------------------------------------------------------------------------------------
def test_calls_without_new_steps_repeat_the_record(engine):
    caps, ns, k = [6, 6, 6], [64, 64, 64], 3
    means, trans = _tables(k, 3, 81)
    obs = _table_observes(means, caps, 81)
    st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans), masses=True)
    empty = [np.zeros(0)] * 3
    none = engine.batch_online_stats(empty)                        # before the first observe
    assert all(np.all(v == 0.0) for v in none.values())
    first = st.check(st.advance((4, 0, 2)))
    assert np.all(first[1] == 0.0), "a problem of length 0 has a zero record"
    again = st.check(empty)                                         # two calls in a row
    assert np.array_equal(again, first)
    blind = engine.batch_online_stats()                             # NULL observes, nothing to consume
    assert np.array_equal(np.stack([_record(blind, b) for b in range(3)]), first)
    st.advance((0, 0, 0))                                           # an advance without observes
    assert np.array_equal(st.check(empty), first)
    # a smoothing call in between counts the new rows; the statistics do not change
    piece = st.advance((2, 3, 0))
    engine.batch_smooth(0)
    later = st.check(piece)
    assert np.array_equal(later[2], first[2]) and not np.array_equal(later[0], first[0])


def test_without_observes_the_weighted_sums_stay_zero(engine):
    caps, ns = [5, 7], [64, 300]
    means, trans = _tables(3, 2, 83)
    obs = _table_observes(means, caps, 83)
    st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans), with_obs=False)
    st.advance((2, 3))
    st.check(None)
    st.advance((3, 4))
    got = st.check(None)
    assert np.all(got[:, 72:] == 0.0) and np.all(got[:, 64:72].sum(axis=1) > 4.9)
    full = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans))
    assert np.array_equal(full.check(full.advance((5, 7)))[:, :72], got[:, :72])


# ---- 4. other k, HMM3, partly filled workgroups ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 9])
@pytest.mark.parametrize("model,k", [(cp.MODEL_HMM_TABLE, 2), (cp.MODEL_HMM_TABLE, 8), (cp.MODEL_HMM3, 3)], ids=["table2", "table8", "hmm3"])
def test_other_k_and_hmm3(engine, model, k, B):
    """B = 1 and 9: a workgroup with one wavefront at work (9: behind two full ones); B = 4: a full workgroup."""
    caps = [3 + (b % 4) for b in range(B)]
    ns = [(1, 64, 300, 1025)[b % 4] for b in range(B)]
    if model == cp.MODEL_HMM3:
        tables, obs = None, [exact.simulate_hmm(caps[b], 300 + b) for b in range(B)]
    else:
        means, trans = _tables(k, B, 91 + k)
        tables, obs = (means, trans), _table_observes(means, caps, 91 + k)
    st = Stream(engine, model, caps, ns, obs, tables, masses=(B == 4))
    st.check(st.advance([min(2, c) for c in caps]))
    got = st.check(st.advance([c - min(2, c) for c in caps]))
    assert st.lens == caps
    assert np.abs(got[:, 64:72].sum(axis=1) - np.array(caps)).max() <= 1e-9


# ---- 5. the defensive rule and absent states --------------------------------------------------------------------------------------
def test_rare_state_runs_the_zero_paths(engine):
    """Problem 1: four particles, observes at state 0's mean, no transition 0 -> 2: generations that hold state 0 alone give
    D[2] = 0 at the step after them, and the last generation lacks a state, so g = 0 at the read-out."""
    caps, ns, k = [12, 12], [300, 4], 3
    means = np.array([[-1.0, 0.5, 2.0], [0.0, 3.0, 10.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.9375, 0.0625, 0.0], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]]])
    rng = np.random.default_rng(5)
    obs = [means[0][rng.integers(0, 3, 12)] + rng.standard_normal(12), 0.1 * rng.standard_normal(12)]
    st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans), masses=True)
    for dT in ((3, 3), (1, 1), (0, 3), (8, 5)):
        st.check(st.advance(dT))
    assert st.P[1][0][2] == 0
    assert st.runs[1].fallbacks >= 1, "no generation of problem 1 held state 0 alone: the defensive rule did not run"
    assert st.runs[1].zero_g >= 1, "every state was present at every read-out of problem 1"


# ---- 6. a long walk ---------------------------------------------------------------------------------------------------------------
def test_long_walk_in_one_call_then_a_few_steps(engine):
    caps, ns, k = [613, 613], [64, 256], 3
    means, trans = _tables(k, 2, 101)
    obs = _table_observes(means, caps, 101)
    st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans), masses=True)
    for dT in ((600, 600), (13, 13)):
        got = st.check(st.advance(dT))
        T = st.lens[0]
        bwd = engine.batch_smooth_stats([obs[b][:T] for b in range(2)])
        for b in range(2):
            back = _record(bwd, b)
            r = float(np.max(np.abs(got[b] - back) / np.maximum(1.0, np.abs(back)))) / (T * 2.0 ** -52)
            print("T = %d, problem %d: forward-only against cpprob_hip_batch_smooth_stats, r = %.4f (bound %.2f)" % (T, b, r, R_BOUND))
            assert r <= R_BOUND


# ---- 7. the device variant --------------------------------------------------------------------------------------------------------
def test_device_variant_behind_the_advance(engine):
    import torch
    caps, ns, k = [7, 12, 3, 12, 12], [64, 300, 1, 5, 1025], 8
    means, trans = _tables(k, 5, 111)
    obs = _table_observes(means, caps, 111)
    schedule = [(3, 0, 1, 5, 2), (0, 4, 2, 0, 3), (4, 8, 0, 7, 7)]
    st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans))
    host = [st.check(st.advance(dT)) for dT in schedule]
    st = Stream(engine, cp.MODEL_HMM_TABLE, caps, ns, obs, (means, trans))
    pad, n_doubles = 256, 5 * 88
    outs, pieces = [], []
    for dT in schedule:                                             # the tensors first: complete before the engine reads them
        flat = np.concatenate([obs[b][st.lens[b]:st.lens[b] + dT[b]] for b in range(5)])
        st.lens = [st.lens[b] + dT[b] for b in range(5)]
        pieces.append(torch.from_numpy(flat).to("cuda:0"))
        outs.append(torch.full((n_doubles + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0"))
    torch.cuda.current_stream().synchronize()
    st.lens = [0] * 5
    for dT, d_obs, d_out in zip(schedule, pieces, outs):           # advance, call, advance, call ...: nothing waits in between
        st.advance(dT)
        engine.batch_online_stats_device(d_out[pad:pad + n_doubles], d_obs)
    engine.sync()
    for i, d_out in enumerate(outs):
        got = d_out.cpu().numpy()
        assert np.all(got[:pad] == 12345.5) and np.all(got[pad + n_doubles:] == 12345.5), "the device variant wrote outside its records"
        assert np.array_equal(got[pad:pad + n_doubles].reshape(5, 88), host[i]), "call %d: the device variant differs from the host call" % i
    assert np.array_equal(engine.batch_online_stats_progress(), np.array(caps, np.uint32))


# ---- 8. refusals and resets -------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_begins_reset():
    import torch
    eng = cp.Engine(0)
    try:
        eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_shapes = 2, 1, 1, 3, None
        for call in (eng.batch_online_stats, eng.batch_online_stats_progress):      # no batch
            with pytest.raises(cp.CpprobHipError) as e:
                call()
            assert e.value.code == ESTATE
        obs = [exact.simulate_hmm(T, 70 + b) for b, T in enumerate([6, 4])]
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])                     # an ordinary batch, begun and run
        for ran in (False, True):
            with pytest.raises(cp.CpprobHipError) as e:
                eng.batch_online_stats()
            assert e.value.code == ESTATE and "online" in str(e.value)
            eng.batch_run(_seeds(2))
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_online_stats_progress()
        assert e.value.code == ESTATE
        eng.batch_begin_online(cp.MODEL_HMM3, [6, 4], [10, 20], _seeds(2), keep_history=False)     # filtering only, no masses
        eng.batch_advance([obs[0][:2], obs[1][:1]])
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_online_stats([obs[0][:2], obs[1][:1]])
        assert e.value.code == ESTATE and "KEEP_MASSES" in str(e.value)

        st = Stream(eng, cp.MODEL_HMM3, [6, 4], [10, 20], obs, masses=True)
        st.check(st.advance((2, 1)))
        piece = st.advance((3, 2))
        flat = np.concatenate(piece)
        rec = np.full(2 * 88, -5.0)
        call = eng.L.cpprob_hip_batch_online_stats
        done = np.array([2, 1], np.uint32)
        for args in ((flat.ctypes.data, flat.size, rec.ctypes.data, rec.size - 1),      # n_doubles < 88 B
                     (flat.ctypes.data, flat.size - 1, rec.ctypes.data, rec.size),      # a wrong n_observes
                     (flat.ctypes.data, flat.size + 1, rec.ctypes.data, rec.size),
                     (None, flat.size, rec.ctypes.data, rec.size),
                     (flat.ctypes.data, flat.size, None, rec.size)):                    # NULL stats
            assert call(eng.h, *args) == EINVAL
            assert np.all(rec == -5.0) and np.array_equal(eng.batch_online_stats_progress(), done)
        d = torch.full((2 * 88,), -9.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        assert eng.L.cpprob_hip_batch_online_stats_device(eng.h, None, 0, C.c_void_p(d.data_ptr()), 2 * 88 - 1) == EINVAL
        assert eng.L.cpprob_hip_batch_online_stats_device(eng.h, None, 0, None, 2 * 88) == EINVAL
        eng.sync()
        assert bool((d == -9.0).all()) and np.array_equal(eng.batch_online_stats_progress(), done)
        st.check(piece, "after the refusals: ")                                         # the bits it would have returned
        # any begin resets the watermark and tau
        st2 = Stream(eng, cp.MODEL_HMM3, [6, 4], [10, 20], obs, masses=True)
        assert np.all(eng.batch_online_stats_progress() == 0)
        st2.check(st2.advance((6, 4)), "after a new begin: ")
    finally:
        eng.close()
