"""Run lanes (include/cpprob_hip.h: cpprob_hip_infer_lanes): cpprob_hip_infer_run calls that follow each other directly are spread
round robin over further streams and workspaces of the context's own.  Every run must compute what it computes on one stream
(CPPROB_HIP_FLAG_SERIAL_RUNS): the same integers and the same doubles, bit for bit, for every form of the step, every sequence of
back-to-back runs, with reads in between, across re-begins, and the lane a run takes must follow the documented rule of the call
sequence alone.
"""
import os

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

SERIAL = cp.capi.FLAG_SERIAL_RUNS
RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED, cp.RESAMPLE_MULTINOMIAL]
SEQUENCES = [1, 2, 3, 4, 7]
HMM5 = (np.array([-2.0, -1.0, 0.0, 1.5, 3.0]),
        np.array([[5, 2, 1, 1, 1], [1, 5, 2, 1, 1], [1, 2, 4, 2, 1], [1, 1, 2, 5, 1], [2, 1, 1, 1, 5]], np.float64))
HMM4 = (np.array([-1.5, 0.0, 1.0, 2.5]), np.array([[4, 1, 1, 1], [1, 4, 1, 1], [1, 1, 4, 1], [1, 1, 1, 4]], np.float64))


@pytest.fixture(scope="module")
def pair():
    """Two contexts of this module's own (the shared one may have handed its stream out): [0] takes lanes, [1] is begun serial."""
    import torch  # noqa: F401
    engs = (cp.Engine(0), cp.Engine(0))
    yield engs
    for e in engs:
        e.close()


@pytest.fixture(scope="module")
def depth(pair, golden_dir):
    """The library's lane depth D: lanes begun after seven back-to-back runs."""
    eng = pair[0]
    eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, _obs(golden_dir, "hmm16", 2), 1000, seed=1)
    for i in range(7):
        eng.run(i)
    d = eng.lanes()["depth"]
    eng.sync()
    assert d in (2, 3, 4)
    return d


def _obs(golden_dir, name, T):
    return np.array(np.load(os.path.join(golden_dir, "observations.npz"))[name][:T])


def _outputs(eng, keep=True, smc=True):
    s, st, ess, res = eng.results()
    out = {"summary": s, "stats": st, "trace": (ess, res), "stats_alone": eng.stats(), "summary_alone": eng.summary(), "trace_alone": eng.step_trace(),
           "logw": eng.logw()}
    if keep:
        out.update(values=eng.values(), paths=eng.paths())
        if smc:
            out.update(ancestors=eng.ancestors())
    return out


def _assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("summary"):
            assert a[k].keys() == b[k].keys()
            for f in a[k]:
                assert np.array_equal(np.asarray(a[k][f]), np.asarray(b[k][f])), (what, k, f, a[k][f], b[k][f])
        elif k.startswith("trace"):
            for x, y in zip(a[k], b[k]):
                assert np.array_equal(np.asarray(x), np.asarray(y)), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


class LaneRule:
    """The documented rule: a run that directly follows another run takes the next lane, round robin; anything else in between and it
    stays where the last run ran (lane 0 after a begin)."""

    def __init__(self, D):
        self.D, self.last, self.chain, self.used = D, 0, False, 0

    def run(self):
        if self.chain:
            self.last = (self.last + 1) % self.D
        self.chain = True
        self.used = max(self.used, self.last)
        return self.last

    def other(self):
        self.chain = False


def _sequence(eng, k, first, mid=None, rule=None, keep=True, smc=True):
    """k back-to-back runs with indices first .. first + k - 1; mid = j: the results are also read after run j.  Returns
    (outputs read in the middle or None, outputs after the last run)."""
    got_mid = None
    for j in range(k):
        eng.run(first + j)
        if rule is not None:
            assert eng.lanes()["last_lane"] == rule.run(), (k, j, mid)
        if mid is not None and j == mid and j + 1 < k:
            got_mid = _outputs(eng, keep, smc)
            if rule is not None:
                rule.other()
                assert eng.lanes()["last_lane"] == rule.last           # (a read moves nothing)
    out = _outputs(eng, keep, smc)
    if rule is not None:
        rule.other()
    return got_mid, out


def _compare_sequences(pair, D, begin, keep=True, smc=True, sequences=SEQUENCES, between=None):
    """begin(eng, flags) begins one context; every sequence runs on both, the lanes' call pattern checked against the rule."""
    lanes, serial = pair
    begin(lanes, 0)
    begin(serial, SERIAL)
    rule = LaneRule(D)
    info = lanes.lanes()
    assert (info["depth"], info["last_lane"], info["serial_reason"]) == (1, 0, 0)
    first = 100
    last = None
    for k in sequences:
        for mid in ([None] if k == 1 else [None, (k - 1) // 2]):
            a_mid, a = _sequence(lanes, k, first, mid, rule, keep, smc)
            b_mid, b = _sequence(serial, k, first, mid, None, keep, smc)
            _assert_same(a, b, (k, mid, "last"))
            if mid is not None:
                _assert_same(a_mid, b_mid, (k, mid, "middle"))
            if last is not None and k > 1:
                assert not np.array_equal(a["logw"], last["logw"]) or a["logw"].size < 4     # (other run indices: other runs)
            last = a
            first += k
        if between is not None and k != sequences[-1]:
            between(lanes, serial)
            rule = LaneRule(D)
    info = lanes.lanes()
    assert serial.lanes()["depth"] == 1 and serial.lanes()["serial_reason"] == cp.capi.SERIAL_FLAG and serial.lanes()["last_lane"] == 0
    assert info["serial_reason"] == 0 and info["depth"] == rule.used + 1
    assert info["lane_bytes"] > 0 or info["depth"] == 1
    return a


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("T", [1, 2, 16])
@pytest.mark.parametrize("n", [1, 1000, 1025, 65537])
def test_lanes_equal_serial_runs_count_form(pair, depth, golden_dir, n, T, rs):
    """hmm<T>, resampling after every step: integer prefix counts; multinomial alternates its strata sets run by run, lane by lane."""
    obs = _obs(golden_dir, "hmm16", T)
    out = _compare_sequences(pair, depth, lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=11, resampler=rs, ess_threshold=2.0, flags=fl))
    assert out["summary"]["step_form"] == cp.capi.FORM_COUNTS
    assert np.allclose(out["stats"].sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("n", [1000, 65537])
def test_lanes_equal_serial_runs_fixed_point_form(pair, depth, golden_dir, n, rs):
    """hmm T = 32 on the ESS schedule: fixed-point masses, resampling only where the ESS falls."""
    obs = _obs(golden_dir, "hmm128", 32)
    out = _compare_sequences(pair, depth, lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=12, resampler=rs, ess_threshold=0.5, flags=fl))
    assert out["summary"]["step_form"] == cp.capi.FORM_FIXED and 0 < out["summary"]["n_resampled"] < 32


@pytest.mark.parametrize("n", [1, 3, 1025])
def test_lanes_equal_serial_runs_repair_on_a_lane(pair, depth, golden_dir, n):
    """One observe 12 standard deviations from every state: where no particle sits in the nearest state (likely with one or three
    particles, out of the question with 1025) the generation loses its bits and is repaired -- on the lane that ran it, at the read."""
    obs = _obs(golden_dir, "hmm128", 32)
    obs[9] = -13.0                                                 # states at -1, 0, 1; -1 is the least visited
    seen = []

    def begin(e, fl):
        e.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=13, ess_threshold=0.5, flags=fl)
    lanes, serial = pair
    begin(lanes, 0)
    begin(serial, SERIAL)
    rule = LaneRule(depth)
    first = 0
    for k in SEQUENCES:
        a_mid, a = _sequence(lanes, k, first, (k - 1) // 2 if k > 1 else None, rule)
        b_mid, b = _sequence(serial, k, first, (k - 1) // 2 if k > 1 else None)
        _assert_same(a, b, (k, "last"))
        if a_mid is not None:
            _assert_same(a_mid, b_mid, (k, "middle"))
        seen.append((lanes.lanes()["last_lane"], a["summary"]["n_requantised"]))
        first += k
    for i in range(12):                                            # pairs of runs: the read visits every lane in turn
        for e in pair:
            e.run(1000 + i)
            e.run(2000 + i)
        rule.run(), rule.run()
        assert lanes.lanes()["last_lane"] == rule.last
        a, b = _outputs(lanes), _outputs(serial)
        rule.other()
        _assert_same(a, b, ("pair", i))
        seen.append((rule.last, a["summary"]["n_requantised"]))
    if n <= 3:
        assert any(lane > 0 and q >= 1 for lane, q in seen), seen       # a repair ran on a further lane


def test_lanes_equal_serial_runs_lgssm_repair(pair, depth, golden_dir):
    """The continuous-weight model, one observe ~30 standard deviations from every particle: every run is repaired at its read."""
    obs = _obs(golden_dir, "lgssm100", 14)
    obs[6] = 40.0
    out = _compare_sequences(pair, depth, lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_LINEAR_GAUSSIAN_1D, obs, 5000, seed=8, ess_threshold=0.5, flags=fl),
                             sequences=[2, 3])
    assert out["summary"]["n_requantised"] >= 1 and out["summary"]["step_form"] == cp.capi.FORM_FIXED


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("n", [1000, 65537])
def test_lanes_equal_serial_runs_lgssm25(pair, depth, golden_dir, n, rs):
    obs = _obs(golden_dir, "lgssm100", 25)
    out = _compare_sequences(pair, depth, lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_LINEAR_GAUSSIAN_1D, obs, n, seed=14, resampler=rs, ess_threshold=0.5, flags=fl))
    assert out["stats"].shape == (25, 2) and np.all(np.isfinite(out["stats"]))


@pytest.mark.parametrize("n", [1, 1025, 65537])
def test_lanes_equal_serial_runs_gaussian_sis(pair, depth, n):
    _compare_sequences(pair, depth, lambda e, fl: e.begin(cp.ALG_SIS, cp.MODEL_GAUSSIAN_UNKNOWN_MEAN, [3.0, 4.0], n, seed=15, flags=fl), smc=False)


@pytest.mark.parametrize("ess", [2.0, 0.5])
@pytest.mark.parametrize("n", [1000, 65537])
def test_lanes_equal_serial_runs_filtering_only(pair, depth, golden_dir, n, ess):
    obs = _obs(golden_dir, "hmm16", 16)
    _compare_sequences(pair, depth, lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=16, ess_threshold=ess, keep_history=False, flags=fl), keep=False)


@pytest.mark.parametrize("n", [1025, 65537])
def test_lanes_equal_serial_runs_hmm_table_across_set_hmm(pair, depth, golden_dir, n):
    """MODEL_HMM_TABLE: the lanes take the context's table; set_hmm and a re-begin between two sequences invalidate them."""
    obs = _obs(golden_dir, "hmm16", 16)
    tables = [HMM5, HMM4]

    def begin(e, fl):
        e.set_hmm(*tables[0])
        e.begin(cp.ALG_SMC, cp.MODEL_HMM_TABLE, obs, n, seed=17, ess_threshold=2.0, flags=fl)

    def between(lanes, serial):
        tables.reverse()
        before = lanes.lanes()["depth"]
        lanes.set_hmm(*tables[0])
        assert lanes.lanes()["depth"] == 1 and lanes.lanes()["last_lane"] == 0 and before >= 1
        with pytest.raises(cp.CpprobHipError):
            lanes.run(0)                                           # (as before: a new table wants a begin)
        begin(lanes, 0)
        begin(serial, SERIAL)

    out = _compare_sequences(pair, depth, begin, sequences=[3, 4], between=between)
    assert out["stats"].shape == (16, 8)


def test_rebegin_with_lanes_at_another_size_and_another_model(pair, depth, golden_dir):
    hmm, lg = _obs(golden_dir, "hmm16", 16), _obs(golden_dir, "lgssm100", 12)
    begins = [lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_HMM3, hmm, 65537, seed=18, flags=fl),
              lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_HMM3, hmm, 1025, seed=18, flags=fl),                                  # smaller: allocations reused
              lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_LINEAR_GAUSSIAN_1D, lg, 4099, seed=18, ess_threshold=0.5, flags=fl),    # another model
              lambda e, fl: e.begin(cp.ALG_SMC, cp.MODEL_HMM3, hmm, 200_001, seed=18, resampler=cp.RESAMPLE_MULTINOMIAL, flags=fl)]  # larger
    lanes, serial = pair
    for b in begins:
        b(lanes, 0)
        assert lanes.lanes()["depth"] == 1 and lanes.lanes()["last_lane"] == 0          # (begun again at their next use)
        b(serial, SERIAL)
        rule = LaneRule(depth)
        _, x = _sequence(lanes, 4, 7, None, rule)
        _, y = _sequence(serial, 4, 7)
        _assert_same(x, y)
        assert lanes.lanes()["depth"] == rule.used + 1 == min(depth, 4)


def test_results_device_reads_the_lane_of_the_last_run(pair, depth, golden_dir):
    import torch
    lanes, serial = pair
    obs = _obs(golden_dir, "hmm16", 16)
    lanes.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 65537, seed=19)
    out = torch.zeros(4 + 16 * 3, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for i in range(3):
        lanes.run(i)
    assert lanes.lanes()["last_lane"] == 2 % depth
    lanes.results_device(out)                                      # (on the context's own stream, behind the lane's run)
    lanes.run(3)                                                   # the lane's next run waits for that copy
    assert lanes.lanes()["last_lane"] == 2 % depth
    lanes.sync()
    got = out.cpu().numpy()
    serial.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 65537, seed=19, flags=SERIAL)
    serial.run(2)
    s, st, _, _ = serial.results()
    assert np.array_equal(got[:4], [s["log_evidence"], s["ess_final"], s["log_norm"], s["max_logw"]])
    assert np.array_equal(got[4:].reshape(16, 3), st)
    lanes.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 65537, seed=19)
    for i in range(3):
        lanes.run(i)
    s2, st2, _, _ = lanes.results()
    assert s2 == s and np.array_equal(st2, st)


def test_lanes_report_depth_and_serial_reasons(golden_dir, depth):
    import torch  # noqa: F401
    obs = _obs(golden_dir, "hmm16", 16)
    eng = cp.Engine(0)
    try:
        assert eng.lanes() == {"depth": 1, "last_lane": 0, "lane_bytes": 0, "serial_reason": 0}
        eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=20)
        eng.run(0)
        eng.results()
        eng.run(1)
        eng.results()
        assert eng.lanes() == {"depth": 1, "last_lane": 0, "lane_bytes": 0, "serial_reason": 0}     # run -> results -> run: nothing allocated
        eng.run(2)
        eng.run(3)
        info = eng.lanes()
        assert info["depth"] == 2 and info["last_lane"] == 1 and info["lane_bytes"] > 0 and info["serial_reason"] == 0
        ref = eng.results()
        # profiling: serial while it is on
        eng.profile_enable(True)
        eng.run(3)
        eng.run(3)
        info = eng.lanes()
        assert info["serial_reason"] == cp.capi.SERIAL_PROFILE and info["last_lane"] == 0
        got = eng.results()
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
        assert eng.profile_read(reset=True)["smc_step"][1] == 32
        eng.profile_enable(False)
        assert eng.lanes()["serial_reason"] == 0
        # a handed-out stream: serial until the context is destroyed
        assert eng.stream_ptr
        eng.run(3)
        eng.run(3)
        info = eng.lanes()
        assert info["serial_reason"] == cp.capi.SERIAL_STREAM and info["last_lane"] == 0
        got = eng.results()
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
        eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=20)
        eng.run(0)
        eng.run(1)
        assert eng.lanes()["serial_reason"] == cp.capi.SERIAL_STREAM and eng.lanes()["depth"] == 1
        eng.sync()
    finally:
        eng.close()
    eng = cp.Engine(0)
    try:
        eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=20, flags=SERIAL)
        eng.run(2)
        eng.run(3)
        assert eng.lanes() == {"depth": 1, "last_lane": 0, "lane_bytes": 0, "serial_reason": cp.capi.SERIAL_FLAG}
        got = eng.results()
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
        # an island shard of a larger population: serial
        eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=20, n_global=40_000, scope=cp.SCOPE_ISLAND)
        eng.run(0)
        eng.run(1)
        assert eng.lanes()["serial_reason"] == cp.capi.SERIAL_SHARD and eng.lanes()["depth"] == 1
        eng.sync()
    finally:
        eng.close()


@pytest.mark.parametrize("why", ["profile", "stream"])
def test_context_pinned_before_its_first_runs_never_begins_a_lane(pair, golden_dir, why):
    """Profiling on, or the stream handed out, BEFORE the first back-to-back runs: depth stays 1, nothing is allocated."""
    obs = _obs(golden_dir, "hmm16", 16)
    serial = pair[1]
    serial.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=23, flags=SERIAL)
    serial.run(4)
    ref = serial.results()
    eng = cp.Engine(0)
    try:
        eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=23)
        if why == "profile":
            eng.profile_enable(True)
        else:
            assert eng.stream_ptr
        for i in range(5):
            eng.run(i)
        reason = cp.capi.SERIAL_PROFILE if why == "profile" else cp.capi.SERIAL_STREAM
        assert eng.lanes() == {"depth": 1, "last_lane": 0, "lane_bytes": 0, "serial_reason": reason}
        got = eng.results()
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
    finally:
        eng.close()


def test_size_rule_at_its_edge(pair, golden_dir):
    """Lanes engage up to 10240 tiles of 1024 particles; one particle more and the context runs one at a time (SERIAL_SIZE)."""
    obs = _obs(golden_dir, "hmm16", 2)
    edge = 10240 * 1024
    serial = pair[1]
    eng = cp.Engine(0)
    try:
        for n, reason in ((edge, 0), (edge + 1, cp.capi.SERIAL_SIZE)):
            eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=24)
            eng.run(0)
            eng.run(1)
            info = eng.lanes()
            assert info["serial_reason"] == reason and info["depth"] == (1 if reason else 2) and info["last_lane"] == (0 if reason else 1)
            assert (info["lane_bytes"] == 0) == bool(reason)
            serial.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=24, flags=SERIAL)
            serial.run(1)
            a, b = eng.results(), serial.results()
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
            eng.close()
            eng = cp.Engine(0)
    finally:
        eng.close()


def test_lane_that_does_not_fit_pins_the_context_serial_without_an_error(pair, golden_dir):
    """The further lanes may hold a quarter of the free device memory.  With all but ~1.5 GB of it reserved elsewhere a 4 10^6-particle
    context (0.5 GB) still begins, its first further lane does not fit: no error, SERIAL_MEMORY, the runs go on one at a time."""
    import torch
    obs = _obs(golden_dir, "hmm16", 16)
    n = 4_000_000
    serial = pair[1]
    serial.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=25, flags=SERIAL)
    serial.run(2)
    ref = serial.results()
    eng = cp.Engine(0)
    filler = None
    try:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        filler = torch.empty(free - (3 << 29), dtype=torch.uint8, device="cuda:0")        # (reserved, never touched)
        eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=25)
        for i in range(3):
            eng.run(i)
        info = eng.lanes()
        assert info == {"depth": 1, "last_lane": 0, "lane_bytes": 0, "serial_reason": cp.capi.SERIAL_MEMORY}
        got = eng.results()
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
        del filler
        filler = None
        torch.cuda.empty_cache()
        eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=25)                           # (pinned until the context is destroyed)
        eng.run(0)
        eng.run(1)
        assert eng.lanes()["serial_reason"] == cp.capi.SERIAL_MEMORY and eng.lanes()["depth"] == 1
        eng.sync()
    finally:
        del filler
        eng.close()
        torch.cuda.empty_cache()


def test_rejected_begin_leaves_the_begun_problem_and_its_lanes(pair, depth, golden_dir):
    """A begin that fails validation changes nothing: the context and its lanes go on with the problem begun before."""
    obs = _obs(golden_dir, "hmm16", 16)
    lanes, serial = pair
    lanes.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=26)
    serial.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=26, flags=SERIAL)
    lanes.run(0)
    lanes.run(1)
    assert lanes.lanes()["depth"] == 2
    with pytest.raises(cp.CpprobHipError):
        lanes.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 20_000, seed=99, resampler=7)
    assert lanes.lanes()["depth"] == 2 and lanes.lanes()["last_lane"] == 1
    for i in (2, 3, 4):
        lanes.run(i)
    assert lanes.lanes()["last_lane"] == (1 + 2) % depth            # (the failed call ended the sequence: run 2 stayed on lane 1)
    serial.run(4)
    _assert_same(_outputs(lanes), _outputs(serial))


def test_own_state_entry_points_wait_for_the_lanes(pair, depth, golden_dir):
    """A building block between two runs ends the sequence (the next run stays on its lane) and leaves the last run's results readable."""
    import torch
    lanes, serial = pair
    obs = _obs(golden_dir, "hmm16", 16)
    lanes.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 65537, seed=21)
    serial.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 65537, seed=21, flags=SERIAL)
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rule = LaneRule(depth)
    for i in range(3):
        lanes.run(i)
        assert lanes.lanes()["last_lane"] == rule.run()
    lanes.draw_normal(5, 0, 0, 0.0, 1.0, buf)
    rule.other()
    lanes.run(3)
    assert lanes.lanes()["last_lane"] == rule.run()
    serial.run(3)
    _assert_same(_outputs(lanes), _outputs(serial))


def test_two_engines_with_lanes_interleaved(pair, depth, golden_dir):
    """Two contexts, each spreading its own back-to-back runs over its own lanes, fed alternately."""
    import torch  # noqa: F401
    obs = _obs(golden_dir, "hmm16", 16)
    engs = [pair[0], cp.Engine(0)]
    try:
        for e in engs:
            e.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 65537, seed=22)
        total = 2 * 7
        for i in range(total):
            engs[i % 2].run(500 + i)
        for e in engs:
            e.sync()
        outs = [_outputs(e) for e in engs]
        assert [e.lanes()["last_lane"] for e in engs] == [6 % depth, 6 % depth]
        assert all(e.lanes()["depth"] == depth for e in engs)
        serial = pair[1]
        serial.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, 65537, seed=22, flags=SERIAL)
        for k, e in enumerate(engs):
            serial.run(500 + total - 2 + k)
            _assert_same(outs[k], _outputs(serial), k)
    finally:
        engs[1].close()
