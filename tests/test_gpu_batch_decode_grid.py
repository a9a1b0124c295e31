"""Decoding a batch at the shapes where the loops of csrc/batch_decode.hpp run more than once: more problems than one workgroup of
batch_decode_forward_kernel holds (blockIdx.x > 0, a last workgroup partly filled, lp, v and tab addressed for b >= 4), row 0 of
batch_decode_trace_kernel over 1, 2, 3, 5, 10 and 258 chunks of 64 words with its state carried from chunk to chunk, the lane items
of its rows blockIdx.y >= 1 on grids of up to 1 + 65 rows, and an online batch whose forward pass resumes at 63, 64, 65, 128 and 129
while the traceback walks words written by different calls.  Every test reads the grids of its call (cpprob_hip_batch_pass_grid) and
asserts the workgroups, rows or chunks it is named for.

References: tests/decode_ref.py on the masses of the rows the run left (or kept) and the library's own log table, as
tests/test_gpu_batch_decode.py.  Paths, fixed-lag rows and scores are pure functions of those bits and IEEE additions: array_equal
and == on doubles, no tolerance.

Left out on purpose: a second trip of the lane rows.  It needs more than 4096 * 256 lane items, a problem of more than 2^20 steps;
at the 0.107 s measured for a run of 16500 steps (profiles/r16_notes.md) that run alone takes about 7 s before any reference is
computed.  tests/test_batch_decode_kernel_text_host.py::test_trace_items_in_several_trips walks those trips on grids it chooses."""
import time

import numpy as np
import pytest

import backward_ref as R
import batch_grid_cases as G
import cpprob_amd as cp
import decode_ref as D

pytestmark = pytest.mark.gpu

LAGS = (0, 3, 64, 600)


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the twins of one trip, the uniform batch and the one-shot batches an online batch is compared with."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _reference(engine, case, kept=False):
    """[(m, ll, lp, lp0, words, path, score)] of the problems of the batch engine has just run."""
    _, Ts, _, means, _, obs, _ = case
    k = means.shape[1]
    out = []
    for b in range(len(Ts)):
        if kept:
            m, ll = G.kept_masses(engine, b, k), R.log_likelihoods(obs[b], means[b])
        else:
            m, ll = G.masses(engine, case, b)
        lp, lp0 = engine.batch_decode_logp(b)
        assert np.all(lp[k:] == -np.inf) and np.all(lp[:, k:] == -np.inf)
        lp = lp[:k, :k].tolist()
        words, v = D.forward(m, ll, lp, lp0)
        path = D.trace(words, len(m) - 1)
        out.append((m, ll, lp, lp0, words, path, v[int(path[-1])]))
    return out


@pytest.fixture(scope="module")
def long_run(engine):
    """The long ragged batch run once with its history kept, and its reference computed once.  A test begins it again (the same
    seeds: the same run) where another batch may have taken the context since."""
    case = G.long_case()
    t0 = time.perf_counter()
    G.begin(engine, case)
    engine.sync()
    t1 = time.perf_counter()
    ref = _reference(engine, case)
    print("the long batch: run %.3f s, references %.3f s" % (t1 - t0, time.perf_counter() - t1))
    return case, ref


def _check_paths(what, paths, score, ref):
    assert len(paths) == len(ref) and score.shape == (len(ref),)
    for b, r in enumerate(ref):
        assert paths[b].dtype == np.int32 and np.array_equal(paths[b], r[5]), "%s, problem %d (L = %d): paths differ, first at step %s" % (
            what, b, len(r[5]), np.flatnonzero(paths[b] != r[5])[:1] if paths[b].shape == r[5].shape else "(shape)")
        assert score[b] == r[6], "%s, problem %d: score %r, reference %r" % (what, b, score[b], r[6])


def _check_lag(what, st, ref, lag, frm=None):
    n_rows = st.shape[1]
    for b, r in enumerate(ref):
        f = 0 if frm is None else frm[b]
        want = D.decode_lag_fast(r[4], lag, f, n_rows)
        assert np.array_equal(st[b], want), "%s, lag %d, problem %d (L = %d, from %d): fixed-lag rows differ, first at row %s" % (
            what, lag, b, len(r[4]), f, np.flatnonzero(st[b] != want)[:1])
        L = len(r[4])
        tail = np.array([t for t in range(max(f, L - 1 - lag), L)], np.int64)      # the rows with e(t) = L - 1: the full decode's
        assert np.array_equal(st[b, tail - f], r[5][tail]), "%s, lag %d, problem %d: the rows whose end is L - 1 are not the full decode's" % (what, lag, b)


# ---- 1. the long ragged batch ------------------------------------------------------------------------------------------------------
def test_full_decode_of_the_long_ragged_batch(engine, long_run):
    """11 problems on three workgroups of the forward kernel, the last with three; row 0 of the traceback over 1, 2, 3, 5, 10 and
    258 chunks."""
    case, ref = long_run
    G.begin(engine, case)
    t0 = time.perf_counter()
    paths, score = engine.batch_decode()
    wall = time.perf_counter() - t0
    G.pass_grid(engine, "full decode", forward=3, trace=1, forecast=0, predictive=0)
    ch = sorted(set(G.chunks(T) for T in case[1]))
    print("full decode: chunks a problem %s, %.3f s wall" % (ch, wall))
    assert ch == [1, 2, 3, 5, 10, 258]
    _check_paths("full decode", paths, score, ref)
    assert all(np.isfinite(r[6]) for r in ref), "a reference score is not finite"
    # the outputs alone, and once more: the scores come from the saved rows, the words are written again
    again, score2 = engine.batch_decode()
    assert all(np.array_equal(x, y) for x, y in zip(paths, again)) and np.array_equal(score, score2)


def test_full_decode_is_not_vacuous(long_run):
    """A lost carry of the traceback's state from chunk to chunk cannot hide behind a path of zeros: in every problem of 300 steps or
    more the reference path is non-zero at some step L - 1 - 64 j, j >= 1 (the state a chunk hands to the next), and takes at least
    two states inside some chunk after the first."""
    case, ref = long_run
    for b, T in enumerate(case[1]):
        if T <= G.K_WAVE:
            continue
        path = ref[b][5]
        borders = np.arange(T - 1 - G.K_WAVE, -1, -G.K_WAVE)
        carried = int(np.count_nonzero(path[borders]))
        mixed = sum(1 for hi in borders if len(set(path[max(hi - G.K_WAVE + 1, 0):hi + 1].tolist())) >= 2)
        states = sorted(set(path.tolist()))
        print("problem %d: L = %d, %d of %d carried states non-zero, %d of %d later chunks with two states or more, states on the path %s" % (
            b, T, carried, borders.size, mixed, borders.size, states))
        if T >= 300:
            assert carried >= 1 and mixed >= 1, "problem %d: choose other observes" % b
    assert any(len(set(ref[b][5].tolist())) >= 3 for b in range(len(ref)))


def test_fixed_lag_rows_over_several_grid_rows(engine, ref_engine, long_run):
    """lag 0, 3, 64 and 600 on all problems: up to 16499 lane items, 1 + 65 grid rows.  The twin on the second context holds the
    problems of at most 600 steps: lag 3 gives problem 7's 596 items 1 + 3 rows, and the same bytes."""
    case, ref = long_run
    G.begin(engine, case)
    Ts = case[1]
    got = {}
    for lag in LAGS:
        t0 = time.perf_counter()
        st, sc = engine.batch_decode_lag(lag)
        wall = time.perf_counter() - t0
        gy, items = G.trace_grid(Ts, lag)
        G.pass_grid(engine, "lag %d, %d lane items" % (lag, items), forward=3, trace=gy)
        print("lag %d: %.3f s wall" % (lag, wall))
        assert gy == {0: 66, 3: 66, 64: 66, 600: 64}[lag]
        assert st.shape == (len(Ts), max(Ts)) and np.array_equal(sc, [r[6] for r in ref])
        _check_lag("long batch", st, ref, lag)
        for b, T in enumerate(Ts):
            assert np.all(st[b, T:] == -1)
        got[lag] = st
    short = G.sub_case(case, G.SHORT)
    G.begin(ref_engine, short)
    for lag in LAGS:
        st, sc = ref_engine.batch_decode_lag(lag)
        gy, items = G.trace_grid(short[1], lag)
        G.pass_grid(ref_engine, "the twin of at most 600 steps, lag %d, %d lane items" % (lag, items), forward=3, trace=gy)
        assert gy == {0: 4, 3: 4, 64: 4, 600: 1}[lag]
        assert np.array_equal(st, got[lag][G.SHORT, :600]) and np.array_equal(sc, [ref[b][6] for b in G.SHORT]), "lag %d: the twin differs" % lag
    assert G.trace_grid(short[1], 3) == (1 + 3, 596)


def test_fixed_lag_rows_from_a_list_on_the_whole_batch(engine, long_run):
    """lag 2: 16497 lane items, 1 + 65 grid rows.  Then a `from` list of 0, L (no row), L - 1, 70 on L = 129 (past a chunk border)
    and 16000 on the long problem."""
    case, ref = long_run
    G.begin(engine, case)
    Ts = case[1]
    st, _ = engine.batch_decode_lag(2)
    gy, items = G.trace_grid(Ts, 2)
    G.pass_grid(engine, "lag 2, %d lane items" % items, forward=3, trace=gy)
    assert (gy, items) == (1 + 65, 16497)
    _check_lag("long batch", st, ref, 2)
    frm = [16000, 1, 62, 0, 64, 128, 70, 0, 1, 299, 23]
    assert all(f <= T for f, T in zip(frm, Ts)) and [b for b in range(len(Ts)) if frm[b] == Ts[b]] == [1, 5, 10]
    t0 = time.perf_counter()
    part, sc = engine.batch_decode_lag(2, frm)
    wall = time.perf_counter() - t0
    gy, items = G.trace_grid(Ts, 2, frm)
    G.pass_grid(engine, "lag 2 from a list, %d lane items" % items, forward=3, trace=gy)
    print("lag 2 from a list: %.3f s wall" % wall)
    assert (gy, items) == (1 + 3, 597) and part.shape == (len(Ts), 600)
    _check_lag("long batch, from a list", part, ref, 2, frm)
    for b, T in enumerate(Ts):
        assert np.array_equal(part[b, :T - frm[b]], st[b, frm[b]:T]) and np.all(part[b, T - frm[b]:] == -1), "problem %d: not the rows of the call from 0" % b
    assert np.array_equal(sc, [r[6] for r in ref])
    # a lag that reaches past a chunk of row 0 on the list: row 0 starts at `from`, inside a chunk
    part, _ = engine.batch_decode_lag(600, frm)
    gy, items = G.trace_grid(Ts, 600, frm)
    G.pass_grid(engine, "lag 600 from a list, %d lane items" % items, forward=3, trace=gy)
    assert gy == 1 and items == 0
    _check_lag("long batch, from a list", part, ref, 600, frm)


def test_keep_masses_batch_returns_the_same_bytes(engine, long_run):
    """The first nine problems, the 16500-step one among them, as a filtering batch that keeps its masses: three workgroups, the last
    with one problem."""
    case, ref = long_run
    nine = G.sub_case(case, list(range(9)))
    frm = [16000, 1, 62, 0, 64, 128, 70, 0, 1]
    G.begin(engine, nine)
    want = (engine.batch_decode(), engine.batch_decode_lag(3), engine.batch_decode_lag(2, frm))
    _check_paths("nine problems, history", want[0][0], want[0][1], ref[:9])
    t0 = time.perf_counter()
    G.begin(engine, nine, keep_history=False, keep_masses=True)
    got = [engine.batch_decode()]
    G.pass_grid(engine, "keep_masses, full decode", forward=3, trace=1)
    got.append(engine.batch_decode_lag(3))
    G.pass_grid(engine, "keep_masses, lag 3", forward=3, trace=G.trace_grid(nine[1], 3)[0])
    got.append(engine.batch_decode_lag(2, frm))
    G.pass_grid(engine, "keep_masses, lag 2 from a list", forward=3, trace=1 + 3)
    print("keep_masses: run and three calls %.3f s wall" % (time.perf_counter() - t0))
    assert all(np.array_equal(x, y) for x, y in zip(got[0][0], want[0][0])) and np.array_equal(got[0][1], want[0][1])
    for i in (1, 2):
        assert np.array_equal(got[i][0], want[i][0]) and np.array_equal(got[i][1], want[i][1])
    for b in (0, 4, 8):
        assert G.kept_masses(engine, b, G.LONG_K) == ref[b][0], "problem %d: the kept masses are not the store's" % b


# ---- 2. a uniform batch: one log table, the thresholds behind the descriptors --------------------------------------------------------
def test_uniform_hmm3_batch_on_three_workgroups(ref_engine):
    """B = 9, T = 130, n = 70 under CPPROB_HIP_MODEL_HMM3: lp_stride = 0 read by problems b >= 4; full, lag 0, lag 3 and scores."""
    case = G.hmm3_case()
    Ts = case[1]
    t0 = time.perf_counter()
    G.begin(ref_engine, case)
    ref = _reference(ref_engine, case)
    paths, score = ref_engine.batch_decode()
    G.pass_grid(ref_engine, "HMM3, full decode", forward=3, trace=1)
    assert G.chunks(Ts[0]) == 3
    _check_paths("HMM3, full decode", paths, score, ref)
    for lag in (0, 3):
        st, sc = ref_engine.batch_decode_lag(lag)
        G.pass_grid(ref_engine, "HMM3, lag %d" % lag, forward=3, trace=2)
        assert np.array_equal(sc, score)
        _check_lag("HMM3", st, ref, lag)
    print("HMM3, B = 9: %.3f s wall" % (time.perf_counter() - t0))
    assert len(set(tuple(r[5].tolist()) for r in ref)) == len(ref), "two problems share a path"
    assert any(np.count_nonzero(r[5][[129 - 64, 129 - 128]]) for r in ref), "every carried state is zero"


# ---- 3. an online batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", [False, True], ids=["history", "keep_masses"])
def test_online_forward_pass_resumes_across_chunk_borders(engine, ref_engine, kept):
    """150 observes fed as 63 + 1 + 1 + 63 + 1 + 21, decoded after every advance: the forward pass resumes from the saved v row at
    63, 64, 65, 128 and 129, and the traceback crosses chunk borders over words written by different calls.  Every output is the
    reference's at that length and the one-shot batch's; fixed-lag rows that are final never change."""
    means, trans, obs, seeds = G.online_case()
    B, k, lag = len(G.ONLINE_CAPS), G.ONLINE_K, 3
    mode = dict(keep_history=False, keep_masses=True) if kept else {}
    t0 = time.perf_counter()
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, G.ONLINE_CAPS, G.ONLINE_NS, seeds, tables=(means, trans), **mode)
    lens = [0] * B
    seen, resumed = [], []
    final = np.full((B, max(G.ONLINE_CAPS)), -1, np.int32)
    for now in G.online_lengths():
        engine.batch_advance([obs[b][lens[b]:now[b]] for b in range(B)])
        resumed.append(lens[0])
        before, lens = lens, now
        paths, score = engine.batch_decode()
        G.pass_grid(engine, "online, lengths %s, full decode" % lens, forward=2, trace=1)
        st, sc = engine.batch_decode_lag(lag)
        G.pass_grid(engine, "online, lengths %s, lag %d" % (lens, lag), forward=2, trace=G.trace_grid(lens, lag)[0])
        assert st.shape == (B, max(lens)) and np.array_equal(sc, score)
        assert paths[G.ONLINE_UNFED].size == 0 and score[G.ONLINE_UNFED] == 0.0 and np.all(st[G.ONLINE_UNFED] == -1)
        frm = [max(L - lag, 0) for L in before]                          # the rows that were not final at the last length
        part, _ = engine.batch_decode_lag(lag, frm)
        for b in range(B):
            L = lens[b]
            assert paths[b].shape == (L,)
            assert np.array_equal(part[b, :L - frm[b]], st[b, frm[b]:L]), "problem %d at length %d: the rows from %d on differ" % (b, L, frm[b])
            done = max(L - lag, 0)
            known = final[b, :done] >= 0
            assert np.array_equal(st[b, :done][known], final[b, :done][known]), "problem %d at length %d: a final row changed" % (b, L)
            final[b, :done] = st[b, :done]
        seen.append((list(lens), paths, score, st))
    assert resumed == [0, 63, 64, 65, 128, 129] and lens == [150, 0, 150, 150, 128, 150]
    print("online (%s): six advances with three decode calls each, %.3f s wall" % ("keep_masses" if kept else "history", time.perf_counter() - t0))
    # the restatement on the masses of the rows reached, at every length
    fed = [b for b in range(B) if b != G.ONLINE_UNFED]
    carried = []
    for b in fed:
        ll = R.log_likelihoods(obs[b][:lens[b]], means[b])
        m = G.kept_masses(engine, b, k) if kept else R.filtering_masses(engine.batch_store(b)[0], ll)
        lp, lp0 = engine.batch_decode_logp(b)
        lp = lp[:k, :k].tolist()
        words, _ = D.forward(m, ll, lp, lp0)
        for at, paths, score, st in seen:
            L = at[b]
            wp, ws = D.decode(m[:L], ll[:L], lp, lp0)
            assert np.array_equal(paths[b], wp) and score[b] == ws, "problem %d, length %d" % (b, L)
            assert np.array_equal(st[b], D.decode_lag_fast(words[:L], lag, 0, st.shape[1])), "problem %d, length %d: fixed-lag rows" % (b, L)
        carried.append(int(np.count_nonzero(wp[np.arange(lens[b] - 1 - G.K_WAVE, -1, -G.K_WAVE)])))
    print("online: carried states that are non-zero, a problem: %s" % carried)
    assert max(carried) >= 1, "every state carried across a chunk border is zero: choose other observes"
    # the one-shot batches of the lengths reached
    for at, paths, score, st in seen:
        ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [obs[b][:at[b]] for b in fed], [G.ONLINE_NS[b] for b in fed], tables=(means[fed], trans[fed]))
        ref_engine.batch_run(seeds[fed])
        p1, s1 = ref_engine.batch_decode()
        G.pass_grid(ref_engine, "one-shot batch of lengths %s" % [at[b] for b in fed], forward=2, trace=1)
        st1, _ = ref_engine.batch_decode_lag(lag)
        for i, b in enumerate(fed):
            assert np.array_equal(paths[b], p1[i]) and score[b] == s1[i], "problem %d, length %d: differs from the one-shot batch" % (b, at[b])
            assert np.array_equal(st[b], st1[i]), "problem %d, length %d: fixed-lag rows differ from the one-shot batch" % (b, at[b])
