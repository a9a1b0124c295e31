"""CPU tests of the plain-Python reference of the trajectory sufficient statistics (tests/trajstats_ref.py; include/cpprob_hip.h:
cpprob_hip_batch_traj_stats): the counting identities of a record, the counting maximum-likelihood tables em.m_step reads from it,
the short problems, and the sums' order."""
import numpy as np
import pytest

import trajstats_ref as TS
from cpprob_amd.em import m_step


@pytest.fixture(scope="module", params=[(2, 7, 1), (5, 64, 2), (8, 301, 3)])
def case(request):
    k, T, seed = request.param
    rng = np.random.default_rng(seed)
    return k, T, rng.integers(0, k, T), rng.uniform(-4.0, 4.0, T)


def test_counts_add_up(case):
    """xi sums to T - 1, occ to T; the transitions leaving a state plus the last state are its visits; states >= k are zero."""
    k, T, path, obs = case
    st = TS.stats(path, obs)
    assert st["xi"].sum() == T - 1 and st["occ"].sum() == T
    last = np.zeros(8)
    last[path[-1]] = 1.0
    assert np.array_equal(st["xi"].sum(axis=1) + last, st["occ"])
    assert np.array_equal(st["occ"], np.bincount(path, minlength=8).astype(np.float64))
    assert np.all(st["xi"][k:] == 0.0) and np.all(st["xi"][:, k:] == 0.0) and all(np.all(st[f][k:] == 0.0) for f in ("occ", "occ_y", "occ_yy"))
    rec = TS.record(st)
    assert rec.shape == (TS.RECORD,) and rec[8 * 1 + 0] == st["xi"][1, 0] and rec[64] == st["occ"][0] and rec[72] == st["occ_y"][0] and rec[87] == st["occ_yy"][7]


def test_sums_run_in_the_walks_order(case):
    """occ_y and occ_yy are sequential sums over t = T-1 .. 0 of the state's own observes -- not a sum in storage order."""
    k, T, path, obs = case
    st = TS.stats(path, obs)
    for s in range(k):
        a = b = 0.0
        for t in range(T - 1, -1, -1):
            if path[t] == s:
                a = a + float(obs[t])
                b = b + float(obs[t]) * float(obs[t])
        assert st["occ_y"][s] == a and st["occ_yy"][s] == b
    blind = TS.stats(path)
    assert np.all(blind["occ_y"] == 0.0) and np.all(blind["occ_yy"] == 0.0) and np.array_equal(blind["xi"], st["xi"])


def test_m_step_on_a_record_gives_the_counting_mle(case):
    """em.m_step reads the record unchanged: transition rows are the transition frequencies, means the states' sample means."""
    k, T, path, obs = case
    st = TS.stats(path, obs)
    means0, trans0 = np.full((1, k), 9.0), np.full((1, k, k), 1.0 / k)
    means, trans = m_step({f: v[None] for f, v in st.items()}, means0, trans0)
    for s in range(k):
        at = np.flatnonzero(path[:-1] == s)
        if at.size:
            freq = np.bincount(path[at + 1], minlength=k) / at.size
            assert np.allclose(trans[0, s], freq, rtol=0, atol=1e-15)
        else:
            assert np.array_equal(trans[0, s], trans0[0, s])
        seen = path == s
        if seen.any():
            assert abs(means[0, s] - obs[seen].mean()) <= 1e-12
        else:
            assert means[0, s] == 9.0


def test_lengths_zero_and_one():
    none = TS.stats([], [])
    assert np.all(TS.record(none) == 0.0)
    one = TS.stats([2], [0.5])
    assert np.all(one["xi"] == 0.0) and one["occ"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and one["occ_y"][2] == 0.5 and one["occ_yy"][2] == 0.25
    assert TS.records(np.zeros((0, 3), np.int32)).shape == (3, 88) and np.all(TS.records(np.zeros((0, 3), np.int32)) == 0.0)
    two = TS.records(np.array([[0, 1], [1, 1]]), [1.0, 2.0])
    assert two[0, 8 * 0 + 1] == 1.0 and two[1, 8 * 1 + 1] == 1.0 and two[:, :64].sum() == 2.0
    assert two[0, 72:74].tolist() == [1.0, 2.0] and two[1, 73] == 3.0 and two[1, 81] == 5.0
