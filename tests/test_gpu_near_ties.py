"""Exact resampling at constructed near-ties (tests/near_ties.py, tests/golden/near_ties.json): every case puts one integer-deciding
comparison of the prefix-count resamplers -- the systematic comb at a particle or a shard bound, the stratified comb's H - F against
u_F, the multinomial threshold against a particle's CDF value, and against a rank's mass bound P_b in the cut launch -- exactly on a
tie or one ulp from it.  One context draws the oracle's ancestors; a loopback group whose shards put P_b on the tie draws the
one-context run's, bit for bit."""
import numpy as np
import pytest

import cpprob_amd as cp
import near_ties as NT

pytestmark = pytest.mark.gpu

CASES = NT.load_cases()
RS = {"systematic": cp.RESAMPLE_SYSTEMATIC, "stratified": cp.RESAMPLE_STRATIFIED, "multinomial": cp.RESAMPLE_MULTINOMIAL, "cut": cp.RESAMPLE_MULTINOMIAL}


def _id(c):
    return "%s-g%d-%s-gap%+d-k%d" % (c["row"], c["gen"], c["position"], c["gap"], c["k"])


def _ctx_paths(g, r, n_r, T):
    e = g.context(r)
    e.n = n_r
    e.T = T
    return e.paths()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_near_tie_one_context_equals_oracle_and_group_equals_one_context(engine, case):
    import torch  # noqa: F401
    from oracle import oracle as O
    obs = np.array([float.fromhex(h) for h in case["obs"]])
    n, seed, rs, T = case["n"], case["seed"], RS[case["row"]], len(case["obs"])
    engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=seed, resampler=rs, ess_threshold=2.0)
    engine.run()
    ref_sum, ref_paths, ref_anc = engine.summary(), engine.paths(), engine.ancestors()
    orc = O.smc(O.MODEL_HMM3, obs, n, seed, rs, 2.0)
    assert np.array_equal(ref_anc, orc["anc"]) and np.array_equal(engine.values(), orc["hist"])
    assert np.array_equal(ref_paths, np.take_along_axis(orc["hist"], O.lineage(orc["anc"]), axis=1))
    assert ref_sum["n_resampled"] == int(orc["resampled"].sum()) == T - 1
    assert abs(ref_sum["log_evidence"] - orc["log_z"]) < 1e-10
    shards = case["shards"]
    g = cp.Group([0] * len(shards))
    g.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=seed, resampler=rs, ess_threshold=2.0, shard_sizes=shards)
    g.run()
    _, s, reruns = g.results()
    paths = np.concatenate([_ctx_paths(g, r, shards[r], T) for r in range(len(shards))], axis=1)
    g.close()
    assert reruns == 0
    assert np.array_equal(paths, ref_paths), "sharded paths differ from the one-context run's (%d columns)" % int((paths != ref_paths).any(axis=0).sum())
    assert s["log_evidence"] == ref_sum["log_evidence"] and s["n_resampled"] == ref_sum["n_resampled"]
