"""tests/decode_ref.py against brute force: every one of the k^T paths over the support is scored by summing its terms in the
recursion's order ((((lp0 + ll_0[x_0]) + lp[x_0][x_1]) + ll_1[x_1]) + ...), one double addition each), and the path is decided from
the back as the recursion decides it: x_{L-1} is the lowest state some path of the largest score ends in; x_{t-1} is the lowest state
s for which some prefix x_0 .. x_{t-1} = s reaches the largest value of score(prefix) + lp[s][x_t].  Addition of doubles is monotone,
so the largest sum over prefixes is the sum of the largest prefix: the enumeration and the dynamic programme must agree to the bit.
No device, no library."""
import itertools
import math

import numpy as np
import pytest

import backward_ref as R
import decode_ref as D

NEG = -math.inf


def _prefix_scores(m, ll, lp, lp0, t):
    """{prefix (x_0 .. x_t): score}, prefixes off the support left out (their score is -inf)."""
    k = len(lp)
    out = {}
    for p in itertools.product(range(k), repeat=t + 1):
        if any(m[i][p[i]] <= 0 for i in range(t + 1)):
            continue
        sc = lp0 + ll[0][p[0]]
        for i in range(1, t + 1):
            sc = sc + lp[p[i - 1]][p[i]]
            sc = sc + ll[i][p[i]]
        out[p] = sc
    return out


def _lowest(cands, k):
    """The lowest state whose candidate is the largest and above -inf, else 0: cands {state: value}."""
    top = max(cands.values(), default=NEG)
    if top == NEG:
        return 0, NEG
    return min(s for s in range(k) if cands.get(s, NEG) == top), top


def brute(m, ll, lp, lp0, e=None):
    """(path x_0 .. x_e, score) of the traceback started at end_e, by enumeration."""
    k = len(lp)
    e = len(m) - 1 if e is None else e
    full = _prefix_scores(m, ll, lp, lp0, e)
    ends = {}
    for p, sc in full.items():
        ends[p[-1]] = max(ends.get(p[-1], NEG), sc)
    x, score = _lowest(ends, k)
    path = [x]
    for t in range(e, 0, -1):
        c = {}
        for p, sc in _prefix_scores(m, ll, lp, lp0, t - 1).items():
            c[p[-1]] = max(c.get(p[-1], NEG), sc + lp[p[-1]][path[0]])
        path.insert(0, _lowest(c, k)[0])
    return np.array(path, np.int32), score


def _problem(rng, k, T, n, trans, identical=False, single=()):
    """(m, ll, lp, lp0): random states and table rows; identical: states 0 and 1 share their rows (every tie goes to 0); single: the
    steps whose particles all sit in one state."""
    v = rng.integers(0, k, (T, n))
    for t in single:
        v[t] = rng.integers(0, k)
    ll = -rng.uniform(0.0, 30.0, (T, k))
    if identical:
        ll[:, 1] = ll[:, 0]
    m = R.filtering_masses(v, ll.tolist())
    lp, lp0 = D.log_table(R.transition_masses(trans))
    return m, ll.tolist(), lp, lp0


def _trans(rng, k, kind):
    tr = rng.uniform(0.05, 1.0, (k, k))
    if kind == "identical":
        tr[1] = tr[0]
        tr[:, 1] = tr[:, 0]
    if kind == "zero":
        tr[0, k - 1] = 0.0
    return tr


CASES = [(k, T, kind) for k in (2, 3) for T in (1, 2, 5, 7) for kind in ("plain", "identical", "zero", "single")]


@pytest.mark.parametrize("k,T,kind", CASES)
def test_reference_is_the_enumerations(k, T, kind):
    rng = np.random.default_rng(100 * k + 10 * T + len(kind))
    for rep in range(3):
        tr = _trans(rng, k, kind)
        single = tuple(range(0, T, 2)) if kind == "single" else ()
        m, ll, lp, lp0 = _problem(rng, k, T, 1 if rep == 0 else 6, tr, kind == "identical", single)
        if kind == "zero":
            assert lp[0][k - 1] == NEG
        path, score = D.decode(m, ll, lp, lp0)
        bp, bs = brute(m, ll, lp, lp0)
        assert np.array_equal(path, bp) and score == bs, (path, bp, score, bs)
        assert all(m[t][path[t]] > 0 for t in range(T)) or score == NEG
        if score > NEG:
            assert all(lp[path[t - 1]][path[t]] > NEG for t in range(1, T)), "a finite path takes no forbidden transition"


def test_ties_go_to_the_lowest_state():
    """Two identical states: the path never names state 1 where state 0 has support."""
    rng = np.random.default_rng(3)
    tr = _trans(rng, 3, "identical")
    m, ll, lp, lp0 = _problem(rng, 3, 7, 40, tr, True)
    m = [[max(r[0], r[1]), max(r[0], r[1]), r[2]] for r in m]         # the two share their support too
    path, _ = D.decode(m, ll, lp, lp0)
    assert not np.any(path == 1)
    assert np.array_equal(path, brute(m, ll, lp, lp0)[0])


def test_all_infinite_column_keeps_zero():
    """A step whose only supported state cannot be reached: the score is -inf, every later backpointer of the column is 0."""
    lp = [[0.0, NEG], [math.log(0.5), math.log(0.5)]]
    m = [[5, 0], [0, 7], [3, 3]]
    ll = [[-1.0, -2.0]] * 3
    words, v = D.forward(m, ll, lp, math.log(0.5))
    assert v == [NEG, NEG] and int(words[2]) == 0 and (int(words[1]) >> 3) & 7 == 0
    path, score = D.decode(m, ll, lp, math.log(0.5))
    assert score == NEG and np.array_equal(path, brute(m, ll, lp, math.log(0.5))[0])


@pytest.mark.parametrize("k", [2, 3])
def test_fixed_lag_rows(k):
    rng = np.random.default_rng(40 + k)
    T = 7
    m, ll, lp, lp0 = _problem(rng, k, T, 5, _trans(rng, k, "plain"), single=(3,))
    words, _ = D.forward(m, ll, lp, lp0)
    full, _ = D.decode(m, ll, lp, lp0)
    for lag in (0, 1, 3, T):
        rows = D.decode_lag(words, lag)
        for t in range(T):
            e = min(t + lag, T - 1)
            assert rows[t] == brute(m, ll, lp, lp0, e)[0][t]
            if t + lag >= T - 1:
                assert rows[t] == full[t]
        # final rows do not change when the sequence is extended; the words of a prefix are the prefix of the words
        for L in range(1, T):
            wl, _ = D.forward(m[:L], ll[:L], lp, lp0)
            assert np.array_equal(wl, words[:L])
            short = D.decode_lag(wl, lag)
            final = [t for t in range(L) if t + lag <= L - 1]
            assert np.array_equal(short[final], rows[final])
        assert np.array_equal(D.decode_lag(words, lag, 2, 9), np.concatenate([rows[2:], np.full(4, -1, np.int32)]))
        # the side-by-side walk is the plain one
        assert np.array_equal(D.decode_lag_fast(words, lag), rows)
        for frm, n_rows in ((2, 9), (0, 3), (T, 2), (T - 1, None)):
            assert np.array_equal(D.decode_lag_fast(words, lag, frm, n_rows), D.decode_lag(words, lag, frm, n_rows))


def test_forward_resumes_from_its_row():
    rng = np.random.default_rng(9)
    m, ll, lp, lp0 = _problem(rng, 3, 7, 9, _trans(rng, 3, "zero"))
    words, v = D.forward(m, ll, lp, lp0)
    for cut in range(0, 8):
        w1, v1 = D.forward(m[:cut], ll[:cut], lp, lp0)
        w2, v2 = D.forward(m, ll, lp, lp0, v1, cut)
        assert np.array_equal(np.concatenate([w1, w2[cut:]]), words) and v2 == v


def test_side_by_side_walk_on_long_rows():
    """Random words of 300 steps (any word is a valid table of back pointers): lags across the 64-word chunk, rows from inside."""
    rng = np.random.default_rng(77)
    words = rng.integers(0, 1 << 27, 300).astype(np.uint32)
    for lag in (0, 2, 63, 64, 65, 299, 300, 1000):
        for frm, n_rows in ((0, None), (70, None), (0, 310), (299, 4)):
            assert np.array_equal(D.decode_lag_fast(words, lag, frm, n_rows), D.decode_lag(words, lag, frm, n_rows)), (lag, frm, n_rows)
