"""A batch advanced in pieces (include/cpprob_hip.h: cpprob_hip_batch_begin_online, _advance, _lengths; csrc/batch_smc.hpp, the RESUME
kernels).  After any sequence of advances, everything the library returns for a problem that has seen L observes must be what a batch
begun by cpprob_hip_batch_begin_problems with that length (same table, particle count and seed) and run once returns: the same
arithmetic in the same order, so integers are compared with array_equal and every double with ==; there is no tolerance anywhere in
this file.  The one-shot batch is pinned to the oracle index for index by tests/test_gpu_batch.py and test_gpu_batch_problems.py."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp
from oracle import exact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED]
# single particle, sub-tile, both sides of a tile edge, multi-pass, the LDS limit
NS = [1, 5, 1023, 1024, 1025, 2048, 4099, 8192]
LENS = [7, 1, 6, 7, 3, 7, 5, 7]
CAPS = [7, 3, 6, 9, 3, 8, 5, 7]                                   # some problems never fill their capacity
B = len(NS)


def _pieces(lens, cuts):
    """Advance a of a schedule given as cumulative lengths: problem b goes from min(cuts[a-1], L_b) to min(cuts[a], L_b)."""
    out, at = [], [0] * len(lens)
    for c in cuts:
        to = [min(c, L) for L in lens]
        out.append([y - x for x, y in zip(at, to)])
        at = to
    return out


SCHEDULES = {
    "whole": [list(LENS)],
    "one_step_each": _pieces(LENS, range(1, 8)),
    "one_then_rest": _pieces(LENS, [1, 7]),
    "rest_then_one": [[L - 1 for L in LENS], [1] * B],
    # problem 3 starts late; every problem but 6 gets nothing in some advance
    "ragged": [[2, 0, 1, 0, 3, 0, 5, 1], [0, 1, 2, 0, 0, 4, 0, 3], [5, 0, 0, 3, 0, 0, 0, 0], [0, 0, 3, 4, 0, 3, 0, 3]],
}
for _name, _s in SCHEDULES.items():
    assert [sum(a[b] for a in _s) for b in range(B)] == LENS, _name


@pytest.fixture(scope="module")
def ref_engine():
    """A second context for the one-shot batches: any begin on `engine` would replace its online batch."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _seeds(nb, base=77):
    return np.array([base + 7919 * b for b in range(nb)], np.uint64)


def _tables(k, nb, seed):
    """tests/test_gpu_batch_problems.py::_tables: table 1 has a zero transition entry."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (nb, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (nb, k, k))
    if nb > 1:
        trans[1, 0, k - 1] = 0.0
    return means, trans


def _problem_set(model, k):
    """(observes of the full lengths, tables or None) of the eight problems."""
    if model == cp.MODEL_HMM3:
        return [exact.simulate_hmm(L, 700 + b) for b, L in enumerate(LENS)], None
    means, trans = _tables(k, B, 300 + k)
    assert (trans == 0.0).sum() == 1
    rng = np.random.default_rng(k)
    return [means[b][rng.integers(0, k, L)] + rng.standard_normal(L) for b, L in enumerate(LENS)], (means, trans)


def _one_shot(ref_engine, model, obs, lens, ns, tables, seeds, rs, keep):
    """The batch of the problems with lens[b] >= 1, begun whole and run once: {b: (summary, stats, ess, res, store or None)}."""
    idx = [b for b, L in enumerate(lens) if L >= 1]
    tb = None if tables is None else (tables[0][idx], tables[1][idx])
    ref_engine.batch_begin_problems(model, [obs[b][:lens[b]] for b in idx], [ns[b] for b in idx], tables=tb, resampler=rs, keep_history=keep)
    ref_engine.batch_run(seeds[idx])
    summ, stats, ess, res = ref_engine.batch_results()
    dev = _results_device(ref_engine, len(idx), stats.shape[1], stats.shape[2])
    return {b: (summ[i], stats[i], ess[i], res[i], ref_engine.batch_store(i) if keep else None, dev[i]) for i, b in enumerate(idx)}


def _results_device(engine, nb, T, spp):
    import torch
    out = torch.full((nb, 4 + T * spp), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_results_device(out)
    engine.sync()
    return out.cpu().numpy()


def _assert_equals_one_shot(engine, ref, lens, keep, note):
    """Every array and summary field of the online batch on `engine` against the one-shot batch `ref` of the lengths reached."""
    assert np.array_equal(engine.batch_lengths(), np.asarray(lens, np.uint32)), note
    summ, stats, ess, res = engine.batch_results()
    T_max, spp = stats.shape[1], stats.shape[2]
    dev = _results_device(engine, len(lens), T_max, spp)
    for b, L in enumerate(lens):
        at = "%s, problem %d (length %d)" % (note, b, L)
        assert summ[b]["n_predict"] == L, at
        # rows a problem has not reached are zero
        assert np.all(stats[b, L:] == 0.0) and np.all(ess[b, L:] == 0.0) and np.all(res[b, L:] == 0), at
        assert np.all(dev[b, 4 + L * spp:] == 0.0), at
        if L == 0:
            continue
        s1, st1, ess1, res1, store1, dev1 = ref[b]
        for f in summ[b]:
            assert summ[b][f] == s1[f], "%s: summary field %s: %r against %r" % (at, f, summ[b][f], s1[f])
        assert np.array_equal(stats[b, :L], st1[:L]), at
        assert np.array_equal(ess[b, :L], ess1[:L]), at
        assert np.array_equal(res[b, :L], res1[:L]), at
        assert np.array_equal(dev[b, :4 + L * spp], dev1[:4 + L * spp]), at
        if keep:
            for name, x, y in zip(("values", "ancestors", "log-weights"), engine.batch_store(b), store1):
                assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), "%s: %s" % (at, name)


def _feed(obs, at, dT):
    return [obs[b][at[b]:at[b] + dT[b]] for b in range(len(obs))]


# ---- 1. pieces equal the whole ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("model,k", [(cp.MODEL_HMM3, 3), (cp.MODEL_HMM_TABLE, 2), (cp.MODEL_HMM_TABLE, 8)])
def test_pieces_equal_the_whole(engine, ref_engine, model, k, rs, keep):
    obs, tables = _problem_set(model, k)
    seeds = _seeds(B, 11 + k)
    whole = _one_shot(ref_engine, model, obs, LENS, NS, tables, seeds, rs, keep)
    for name, schedule in SCHEDULES.items():
        engine.batch_begin_online(model, CAPS, NS, seeds, tables=tables, resampler=rs, keep_history=keep)
        assert np.array_equal(engine.batch_lengths(), np.zeros(B, np.uint32))
        at = [0] * B
        for a, dT in enumerate(schedule):
            engine.batch_advance(_feed(obs, at, dT))
            at = [x + y for x, y in zip(at, dT)]
            if name == "ragged" and a + 1 < len(schedule):
                # after every advance: the one-shot batch of the lengths reached so far
                _assert_equals_one_shot(engine, _one_shot(ref_engine, model, obs, at, NS, tables, seeds, rs, keep), at, keep, "%s after advance %d" % (name, a))
        assert at == LENS
        _assert_equals_one_shot(engine, whole, LENS, keep, name)


# ---- 2. the requantise branch crosses a junction ------------------------------------------------------------------------------------
def test_requantised_generations_on_both_sides_of_a_junction(engine, ref_engine):
    """tests/test_gpu_batch.py::test_requantised_generations_resample_like_the_one_problem_engine's construction: after step 0 both
    surviving states sit far below every step's bound, so every generation from 1 on is weighed against its exact maximum -- the last
    one of a piece (whose count the next piece rewinds and takes again) and the first one of the next alike."""
    means, trans = [-1.0, 0.0, 10.0], [[5.0, 5.0, 0.01], [5.0, 5.0, 0.01], [1.0, 1.0, 1.0]]
    engine.set_hmm(means, trans)
    ref_engine.set_hmm(means, trans)
    T, nb = 8, 4
    obs = np.full((nb, T), 30.0)
    obs[:, 0] = [-0.5, -1.2, 0.3, -0.1]
    seeds = _seeds(nb, 41)
    for n in (3, 8):
        for rs in RESAMPLERS:
            for keep in (True, False):
                whole = _one_shot(ref_engine, cp.MODEL_HMM_TABLE, list(obs), [T] * nb, [n] * nb, None, seeds, rs, keep)
                assert all(whole[b][0]["n_requantised"] >= T - 2 for b in range(nb)), [whole[b][0]["n_requantised"] for b in range(nb)]
                for cuts in ([3, 8], [4, 5, 8], list(range(1, 9))):
                    engine.batch_begin_online(cp.MODEL_HMM_TABLE, [T] * nb, n, seeds, resampler=rs, keep_history=keep)
                    at = [0] * nb
                    for dT in _pieces([T] * nb, cuts):
                        engine.batch_advance(_feed(list(obs), at, dT))
                        at = [x + y for x, y in zip(at, dT)]
                    summ = engine.batch_results()[0]
                    for b in range(nb):
                        assert summ[b]["n_requantised"] == whole[b][0]["n_requantised"] and summ[b]["max_logw"] == whole[b][0]["max_logw"]
                        if keep:
                            assert np.array_equal(engine.batch_store(b)[1], whole[b][4][1])
                    _assert_equals_one_shot(engine, whole, [T] * nb, keep, "cuts %s" % cuts)


# ---- 3. near ties at a junction -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["systematic", "stratified"])
def test_near_ties_at_a_junction(engine, row):
    """tests/golden/near_ties_batch.json (generation 0 or 1, T = 3): the comb decision on a tie or one ulp from it is the resampling
    of generation `gen`, taken here by the piece that RESUMES after it -- the advance boundary sits right after that generation.
    Every problem draws the oracle's ancestors, as tests/test_gpu_batch.py checks for the one-shot batch."""
    import near_ties_batch as NB
    cases = [c for c in NB.load_cases() if c["row"] == row]
    assert cases and {c["gen"] for c in cases} == {0, 1} and NB.T == 3
    rs = cp.RESAMPLE_SYSTEMATIC if row == "systematic" else cp.RESAMPLE_STRATIFIED
    obs = np.array([[float.fromhex(h) for h in c["obs"]] for c in cases])
    assert obs.shape == (len(cases), NB.T)
    seeds = np.array([c["seed"] for c in cases], np.uint64)
    first = [c["gen"] + 1 for c in cases]
    engine.batch_begin_online(cp.MODEL_HMM3, [NB.T] * len(cases), NB.N, seeds, resampler=rs)
    engine.batch_advance([obs[b][:first[b]] for b in range(len(cases))])
    assert np.array_equal(engine.batch_lengths(), np.asarray(first, np.uint32))
    engine.batch_advance([obs[b][first[b]:] for b in range(len(cases))])
    summ = engine.batch_results()[0]
    for b, c in enumerate(cases):
        vals, anc, _ = engine.batch_store(b)
        orc = O.smc(O.MODEL_HMM3, obs[b], NB.N, c["seed"], rs, 2.0)
        assert np.array_equal(vals, orc["hist"]), c
        assert np.array_equal(anc, orc["anc"]), "%s gen %d %s gap %+d: ancestors differ from the oracle" % (row, c["gen"], c["position"], c["gap"])
        assert abs(summ[b]["log_evidence"] - orc["log_z"]) < 1e-10          # (test_near_ties_at_the_batch_kernels_partition_edges' own bound)


# ---- 4. readout = 0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [(cp.MODEL_HMM3, 3), (cp.MODEL_HMM_TABLE, 8)])
def test_an_advance_without_read_out_defers_the_statistics(engine, ref_engine, model, k):
    import torch
    obs, tables = _problem_set(model, k)
    seeds = _seeds(B, 5)
    rs = cp.RESAMPLE_SYSTEMATIC
    whole = _one_shot(ref_engine, model, obs, LENS, NS, tables, seeds, rs, True)
    engine.batch_begin_online(model, CAPS, NS, seeds, tables=tables, resampler=rs)
    at = [0] * B
    for dT in SCHEDULES["ragged"]:
        engine.batch_advance(_feed(obs, at, dT), readout=False)
        at = [x + y for x, y in zip(at, dT)]
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_results()
    assert e.value.code == ESTATE
    out = torch.zeros((B, 4 + max(CAPS) * (3 if model == cp.MODEL_HMM3 else 8)), dtype=torch.float64, device="cuda:0")
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_results_device(out)
    assert e.value.code == ESTATE
    # summaries, ESS, flags and the store are served, and are the one-shot's
    summ, stats, ess, res = engine.batch_results(with_stats=False)
    assert stats is None
    for b, L in enumerate(LENS):
        assert summ[b] == whole[b][0]
        assert np.array_equal(ess[b, :L], whole[b][2][:L]) and np.array_equal(res[b, :L], whole[b][3][:L])
        for x, y in zip(engine.batch_store(b), whole[b][4]):
            assert np.array_equal(x, y)
    # an advance without observes and with the read-out: the walk and nothing else
    engine.batch_advance([[] for _ in range(B)], readout=True)
    _assert_equals_one_shot(engine, whole, LENS, True, "after the deferred read-out")
    # filtering batches keep every row as they go: readout is ignored
    whole0 = _one_shot(ref_engine, model, obs, LENS, NS, tables, seeds, rs, False)
    engine.batch_begin_online(model, CAPS, NS, seeds, tables=tables, resampler=rs, keep_history=False)
    engine.batch_advance(_feed(obs, [0] * B, LENS), readout=False)
    _assert_equals_one_shot(engine, whole0, LENS, False, "filtering, readout = 0")


# ---- 5. state rules -----------------------------------------------------------------------------------------------------------------
def test_state_rules(engine, ref_engine):
    model = cp.MODEL_HMM3
    obs, _ = _problem_set(model, 3)
    seeds = _seeds(B, 3)
    whole = _one_shot(ref_engine, model, obs, LENS, NS, None, seeds, cp.RESAMPLE_STRATIFIED, True)
    engine.batch_begin_online(model, CAPS, NS, seeds, resampler=cp.RESAMPLE_STRATIFIED)
    first = [2, 0, 1, 0, 3, 0, 5, 1]
    engine.batch_advance(_feed(obs, [0] * B, first))
    # over capacity: refused, naming the problem, and nothing changes
    over = [0] * B
    over[4] = CAPS[4] - first[4] + 1
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_advance([np.zeros(d) for d in over])
    assert e.value.code == EINVAL and "problem 4" in str(e.value)
    assert np.array_equal(engine.batch_lengths(), np.asarray(first, np.uint32))
    # an online batch is advanced, not run
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_run(seeds)
    assert e.value.code == ESTATE
    # a single-population run between two advances changes nothing
    single = exact.simulate_hmm(12, 1)
    engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, single, 5000, seed=9, ess_threshold=2.0)
    engine.run(0)
    s_single = engine.results()[0]
    rest = [L - f for L, f in zip(LENS, first)]
    engine.batch_advance(_feed(obs, first, rest))
    _assert_equals_one_shot(engine, whole, LENS, True, "around a single-population run")
    assert engine.results()[0] == s_single
    ws = cp.capi.batch_online_workspace_bytes(model, CAPS, NS, resampler=cp.RESAMPLE_STRATIFIED)
    assert ws > cp.capi.batch_problems_workspace_bytes(model, CAPS, NS, resampler=cp.RESAMPLE_STRATIFIED)
    # a described batch is run, not advanced; it replaces the online batch
    engine.batch_begin_problems(model, obs, NS)
    for call in (lambda: engine.L.cpprob_hip_batch_advance(engine.h, np.zeros(B, np.uint32).ctypes.data_as(cp.capi.C.POINTER(cp.capi.C.c_uint32)), None, 1),
                 lambda: engine.L.cpprob_hip_batch_lengths(engine.h, np.zeros(B, np.uint32).ctypes.data_as(cp.capi.C.POINTER(cp.capi.C.c_uint32)))):
        assert call() == ESTATE
    # a uniform batch on the same context afterwards still equals its own reference (the workspace only grows)
    T, n, nb = 6, 1500, 5
    uni = np.stack([exact.simulate_hmm(T, 40 + b) for b in range(nb)])
    ref_engine.batch_begin(model, uni, n)
    ref_engine.batch_run(seeds[:nb])
    want = ref_engine.batch_results()
    engine.batch_begin(model, uni, n)
    engine.batch_run(seeds[:nb])
    got = engine.batch_results()
    assert got[0] == want[0] and all(np.array_equal(x, y) for x, y in zip(got[1:], want[1:]))
    for b in range(nb):
        assert all(np.array_equal(x, y) for x, y in zip(engine.batch_store(b), ref_engine.batch_store(b)))


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------
def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def test_cpprob_main_stream_chunk_prints_the_one_shot_output(engine, tmp_path):
    """cpprob_main --batch_tables_file F --stream_chunk 3 (cpprob::gpu::HmmTableStream: the observes fed three a problem at a time,
    the read-out with the last advance only) prints byte for byte what the same command prints without --stream_chunk."""
    main = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
    Ts, k, n, seed = [7, 3, 10, 1, 4], 4, 3000, 40
    means, trans = _tables(k, len(Ts), 55)
    rng = np.random.default_rng(6)
    obs = [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(len(Ts))))
    base = [main, "--model_folder", str(tmp_path), "--smc", "--n_samples", str(n), "--seed", str(seed), "--ess_threshold", "2.0", "--batch_tables_file", "tables.txt"]
    one = subprocess.run(base, capture_output=True, timeout=600)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    assert len(one.stdout.splitlines()) == len(Ts)
    for chunk in ("3", "100"):
        pieces = subprocess.run(base + ["--stream_chunk", chunk], capture_output=True, timeout=600)
        assert pieces.returncode == 0, pieces.stdout[-2000:] + pieces.stderr[-2000:]
        assert pieces.stdout == one.stdout, chunk
