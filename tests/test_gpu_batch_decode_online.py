"""Decoding an online batch (cpprob_hip_batch_decode, cpprob_hip_batch_decode_lag on a batch begun with
cpprob_hip_batch_begin_online): a 37-step stream fed one observe at a time, as 5 + 0 + 17 + 15 and at once, with the history kept and
with the masses kept.  The step words are kept across advances, so every output must be the one the whole stream gives at that length:
equal to tests/decode_ref.py on the masses of the rows reached, the same for every cut, final rows never changing, and untouched by the
smoothing and forecast calls that share the counting watermark."""
import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import decode_ref as D
from oracle import exact

pytestmark = pytest.mark.gpu

L_END, LAG = 37, 4
CUTS = {"37x1": [1] * 37, "5+0+17+15": [5, 0, 17, 15], "at once": [37]}
CAPS, NS = [37, 9, 40], [100, 3, 300]
FED = (0, 2)                                                       # problem 1 never sees an observe: length 0 throughout


def _seeds(nb, base=11):
    return np.array([base + 7919 * b for b in range(nb)], np.uint64)


def _problem(model):
    """(tables or None, means [3, k], observes, k)."""
    if model == cp.MODEL_HMM3:
        return None, np.array([exact.HMM_MEAN] * 3), [exact.simulate_hmm(L_END, 60 + b) for b in range(3)], 3
    rng = np.random.default_rng(41)
    k = 5
    means = np.sort(rng.uniform(-3.0, 3.0, (3, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (3, k, k))
    trans[2, 0, k - 1] = 0.0
    return (means, trans), means, [means[b][rng.integers(0, k, L_END)] + rng.standard_normal(L_END) for b in range(3)], k


def _mode(kept):
    return dict(keep_history=False, keep_masses=True) if kept else {}


def _feed(engine, obs, lo, hi):
    engine.batch_advance([obs[b][lo:hi] if b in FED else np.zeros(0) for b in range(3)])


@pytest.mark.parametrize("kept", [False, True], ids=["history", "keep_masses"])
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE], ids=["hmm3", "table5"])
def test_cuts_agree_and_are_the_references(engine, model, kept):
    tables, means, obs, k = _problem(model)
    seen = {}                                                      # length -> (paths, score, fixed-lag rows) of the first cut that reached it
    for name, cut in CUTS.items():
        engine.batch_begin_online(model, CAPS, NS, _seeds(3), tables=tables, **_mode(kept))
        paths, score = engine.batch_decode()                       # no observes yet
        assert all(p.size == 0 for p in paths) and np.all(score == 0.0)
        st, _ = engine.batch_decode_lag(LAG)
        assert st.shape == (3, 0)
        L = 0
        final = np.full((3, L_END), -1, np.int32)                  # the fixed-lag rows that are final so far
        for dT in cut:
            _feed(engine, obs, L, L + dT)
            L += dT
            paths, score = engine.batch_decode()
            st, sc = engine.batch_decode_lag(LAG)
            assert st.shape == (3, L) and np.array_equal(sc, score)
            assert paths[1].size == 0 and score[1] == 0.0 and np.all(st[1] == -1)
            for b in FED:
                assert paths[b].shape == (L,)
                tail = [t for t in range(L) if t + LAG >= L - 1]
                assert np.array_equal(st[b, tail], paths[b][tail]), "%s, length %d: the rows whose end is L - 1 are the full decode's" % (name, L)
                done = max(L - LAG, 0)
                known = final[b, :done] >= 0
                assert np.array_equal(st[b, :done][known], final[b, :done][known]), "%s, length %d: a final row changed" % (name, L)
                final[b, :done] = st[b, :done]
            if L in seen:
                assert all(np.array_equal(x, y) for x, y in zip(paths, seen[L][0])), "%s, length %d: the cut changed a path" % (name, L)
                assert np.array_equal(score, seen[L][1]) and np.array_equal(st, seen[L][2]), "%s, length %d" % (name, L)
            else:
                seen[L] = (paths, score, st)
            if L and L < L_END:                                    # asking from a later step on: the same rows
                part, _ = engine.batch_decode_lag(LAG, [max(L - 2, 0), 0, L])
                assert np.array_equal(part[0, :min(L, 2)], st[0, max(L - 2, 0):]) and np.all(part[2] == -1)
        assert L == L_END
    # the restatement, on the masses of the rows reached and the library's table
    for b in FED:
        ll = R.log_likelihoods(obs[b], means[b])
        m = [[int(x) for x in row[:k]] for row in engine.batch_masses(b)] if kept else R.filtering_masses(engine.batch_store(b)[0], ll)
        lp, lp0 = engine.batch_decode_logp(b)
        lp = lp[:k, :k].tolist()
        words, _ = D.forward(m, ll, lp, lp0)
        for L, (paths, score, st) in seen.items():
            wp, ws = D.decode(m[:L], ll[:L], lp, lp0)
            assert np.array_equal(paths[b], wp) and score[b] == ws, "problem %d, length %d" % (b, L)
            assert np.array_equal(st[b], D.decode_lag(words[:L], LAG, 0, L)), "problem %d, length %d: fixed-lag rows" % (b, L)


def _session(engine, model, tables, obs, kept, decode, smooth):
    """Advance 5, advance 17, advance 15 with decode calls and / or smoothing and forecast calls after each: what each kind returns."""
    engine.batch_begin_online(model, CAPS, NS, _seeds(3), tables=tables, **_mode(kept))
    dec, sm = [], []
    L = 0
    for dT in (5, 17, 15):
        _feed(engine, obs, L, L + dT)
        L += dT
        if decode and L != 22:                                     # (the second advance's steps are decoded with the third's: the
            dec.append(engine.batch_decode_lag(LAG))               # counting watermark runs ahead of the decode's)
        if smooth:
            sm.append((engine.batch_smooth_lag(2, n_traj=5), engine.batch_forecast(3, 9)))
        if decode and L != 22:
            dec.append(engine.batch_decode())
    if smooth:
        sm.append((engine.batch_smooth(5), engine.batch_predictive()))
    return dec, sm


@pytest.mark.parametrize("kept", [False, True], ids=["history", "keep_masses"])
def test_smoothing_calls_between_decodes_change_nothing(engine, kept):
    tables, _, obs, _ = _problem(cp.MODEL_HMM_TABLE)
    both = _session(engine, cp.MODEL_HMM_TABLE, tables, obs, kept, True, True)
    dec = _session(engine, cp.MODEL_HMM_TABLE, tables, obs, kept, True, False)[0]
    sm = _session(engine, cp.MODEL_HMM_TABLE, tables, obs, kept, False, True)[1]

    def same(x, y):
        if isinstance(x, (tuple, list)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        return np.array_equal(x, y)
    assert len(both[0]) == 4 and same(both[0], dec), "the smoothing calls changed a decode"
    assert len(both[1]) == 4 and same(both[1], sm), "the decode calls changed a smoothing result"
