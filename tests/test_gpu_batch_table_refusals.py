"""What the ten table-taking entry points of the raw library answer, call by call (include/cpprob_hip.h: cpprob_hip_batch_begin_problems,
_begin_online, _retable, _retable_device, _online_tables and their _scaled forms): the return code and the text of
cpprob_hip_last_error, in seven states of a context, for good arguments and for each defect a caller can hand in, double defects
included -- they fix which refusal comes first.  The table below is written out from the library's refusals as they stood before the
unit and scaled host routes were folded into one; the folded routes answer the same.  A refused call changes nothing: the batch's
results before the refusals and after them are equal, and a call that succeeds leaves a batch that computes what the state's own begin
computes.  (A successful call leaves the error text as it was: only the code is tabled for it.)

Two problems of 3 and 2 observes, 2 states, 8 particles each, with a particle store."""
import ctypes as C

import numpy as np
import pytest

import cpprob_amd as cp
import cpprob_amd.capi as capi
import devmem

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -3, -4
P32, P64, PD = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)

LENGTHS = np.array([3, 2], np.uint32)
PARTICLES = np.array([8, 8], np.uint32)
MEANS = np.array([[-1.0, 1.0], [-0.5, 1.5]])
TRANS = np.array([[[0.9, 0.1], [0.2, 0.8]], [[0.7, 0.3], [0.4, 0.6]]])
SIGMAS = np.array([[1.0, 0.5], [2.0, 1.5]])
OBS = np.array([0.5, -1.25, 1.0, 1.75, -0.5])                 # problem 0's three observes, then problem 1's two
SEEDS = np.array([11, 12], np.uint64)
FIRST, REST = np.array([2, 1], np.uint32), np.array([1, 1], np.uint32)      # an online batch's two advances

STATES = ("none", "uniform", "unit", "scaled", "online unit", "online scaled", "hmm3")

# ---- the table -----------------------------------------------------------------------------------------------------------------------
OK = (0, None)
NULL = (EINVAL, "NULL argument")
BOTH = (EINVAL, "per-problem tables need both h_means and h_transition")
WEIGHT = (EINVAL, "problem 1: transition weights must be finite and >= 0")
MEAN = (EINVAL, "problem 0: state means must be finite")
SCALE = (EINVAL, "problem 1: emission scales must be finite and > 0, with a normal finite 2 pi sigma^2")
NO_OBSERVES = (EINVAL, "h_observes is NULL and no re-table of this begun batch has staged the observes")
COUNT = (EINVAL, "n_observes = 6, the problems' lengths sum to 5")
SERVE = (EUNSUPPORTED, "emission scales serve CPPROB_HIP_MODEL_HMM_TABLE with per-problem tables")
NOT_BEGUN = (ESTATE, "no batch is begun")
SHARED = (EUNSUPPORTED, "a batch begun by cpprob_hip_batch_begin shares one table: begin it with cpprob_hip_batch_begin_problems to re-table it")
ONLINE = (EUNSUPPORTED, "an online batch is not re-tabled: its advances evaluate their rows from the host's means")
MODELS = (EUNSUPPORTED, "re-tabling serves CPPROB_HIP_MODEL_HMM_TABLE: the table of CPPROB_HIP_MODEL_HMM3 is the model's")
HAS_SCALES = (ESTATE, "the batch has emission scales: it is re-tabled by cpprob_hip_batch_retable_scaled / _retable_scaled_device")
NO_SCALES = (ESTATE, "the batch has no emission scales: begin it with cpprob_hip_batch_begin_problems_scaled, or re-table it with cpprob_hip_batch_retable / _retable_device")
ONLINE_HAS_SCALES = (ESTATE, "the batch has emission scales: its tables are replaced by cpprob_hip_batch_online_tables_scaled")
ONLINE_NO_SCALES = (ESTATE, "the batch has no emission scales: begin it with cpprob_hip_batch_begin_online_scaled, or call cpprob_hip_batch_online_tables")
NOT_ONLINE = (ESTATE, "cpprob_hip_batch_online_tables serves a batch begun by cpprob_hip_batch_begin_online")
NOT_ONLINE_SCALED = (ESTATE, "cpprob_hip_batch_online_tables_scaled serves a batch begun by cpprob_hip_batch_begin_online")
NOT_RUN = (ESTATE, "cpprob_hip_batch_begin has not been called")

# a begin answers the same in every state
BEGIN = {"good": OK, "means NULL": BOTH, "transition NULL": BOTH, "weight": WEIGHT, "mean": MEAN}
BEGIN_SCALED = {"good": OK, "means NULL": NULL, "transition NULL": NULL, "sigmas NULL": NULL, "weight": WEIGHT, "mean": MEAN, "sigma zero": SCALE,
                "sigma subnormal": SCALE, "weight + sigma zero": WEIGHT, "HMM3, no problems": SERVE}
# a re-table outside the two described HMM_TABLE states: one answer, whatever the arguments
ELSEWHERE = {"none": NOT_BEGUN, "uniform": SHARED, "online unit": ONLINE, "online scaled": ONLINE, "hmm3": MODELS}
HOST = {"good": OK, "means NULL": NULL, "transition NULL": NULL, "observes NULL": NO_OBSERVES, "count": COUNT, "weight": WEIGHT, "mean": MEAN,
        "observes NULL + weight": NO_OBSERVES}
HOST_SCALED = dict(HOST, **{"sigmas NULL": NULL, "sigma zero": SCALE, "sigma subnormal": SCALE, "weight + sigma zero": WEIGHT})
DEVICE = {"good": OK, "means NULL": NULL, "transition NULL": NULL, "observes NULL": NULL, "count": COUNT}
DEVICE_SCALED = dict(DEVICE, **{"sigmas NULL": NULL})
TABLES = {"good": OK, "means NULL": NULL, "transition NULL": NULL, "weight": WEIGHT, "mean": MEAN}
TABLES_SCALED = dict(TABLES, **{"sigmas NULL": NULL, "sigma zero": SCALE, "sigma subnormal": SCALE, "weight + sigma zero": WEIGHT})
OFFLINE = ("none", "uniform", "unit", "scaled", "hmm3")

# TABLE[entry point][state]: one answer for every call, or the answer by defect.  (A scaled re-table of a unit batch with NULL sigmas is
# NO_SCALES, not NULL: the state is judged before the arguments.)
TABLE = {
    "begin_problems": {s: BEGIN for s in STATES},
    "begin_problems_scaled": {s: BEGIN_SCALED for s in STATES},
    "begin_online": {s: BEGIN for s in STATES},
    "begin_online_scaled": {s: BEGIN_SCALED for s in STATES},
    "retable": dict(ELSEWHERE, unit=HOST, scaled=HAS_SCALES),
    "retable_scaled": dict(ELSEWHERE, unit=NO_SCALES, scaled=HOST_SCALED),
    "retable_device": dict(ELSEWHERE, unit=DEVICE, scaled=HAS_SCALES),
    "retable_scaled_device": dict(ELSEWHERE, unit=NO_SCALES, scaled=DEVICE_SCALED),
    "online_tables": dict({s: NOT_ONLINE for s in OFFLINE}, **{"online unit": TABLES, "online scaled": ONLINE_HAS_SCALES}),
    "online_tables_scaled": dict({s: NOT_ONLINE_SCALED for s in OFFLINE}, **{"online unit": ONLINE_NO_SCALES, "online scaled": TABLES_SCALED}),
}
# the defects every entry point is called with, in every state
DEFECTS = {"begin_problems": BEGIN, "begin_problems_scaled": BEGIN_SCALED, "begin_online": BEGIN, "begin_online_scaled": BEGIN_SCALED, "retable": HOST,
           "retable_scaled": HOST_SCALED, "retable_device": DEVICE, "retable_scaled_device": DEVICE_SCALED, "online_tables": TABLES, "online_tables_scaled": TABLES_SCALED}
# the state whose own begin computes what a batch begun by this entry point computes
BEGINS_AS = {"begin_problems": "unit", "begin_problems_scaled": "scaled", "begin_online": "online unit", "begin_online_scaled": "online scaled"}


def test_the_table_covers_every_entry_point_in_every_state():
    assert set(TABLE) == set(DEFECTS) and len(TABLE) == 10
    for fn, rows in TABLE.items():
        assert set(rows) == set(STATES), fn
        for state, row in rows.items():
            assert isinstance(row, tuple) or set(row) == set(DEFECTS[fn]), (fn, state)


# ---- the calls ---------------------------------------------------------------------------------------------------------------------------
def _arguments(defect):
    """Good arguments, broken as the defect says."""
    a = {"means": MEANS.copy(), "trans": TRANS.copy(), "sigmas": SIGMAS.copy(), "obs": OBS.copy(), "n_obs": OBS.size, "model": cp.MODEL_HMM_TABLE, "n_problems": 2}
    for d in defect.split(" + "):
        if d == "means NULL":
            a["means"] = None
        elif d == "transition NULL":
            a["trans"] = None
        elif d == "sigmas NULL":
            a["sigmas"] = None
        elif d == "observes NULL":
            a["obs"] = None
        elif d == "count":
            a["n_obs"] = OBS.size + 1
        elif d == "weight":
            a["trans"][1, 1, 0] = -0.25
        elif d == "mean":
            a["means"][0, 1] = np.inf
        elif d == "sigma zero":
            a["sigmas"][1, 0] = 0.0
        elif d == "sigma subnormal":
            a["sigmas"][1, 1] = 1e-160                        # (2 pi sigma^2 = 6.3e-320)
        elif d == "HMM3, no problems":
            a["model"], a["n_problems"] = cp.MODEL_HMM3, 0
        else:
            assert d == "good", d
    return a


def _p(x):
    return None if x is None else x.ctypes.data


def _config(model=cp.MODEL_HMM_TABLE, n_problems=2):
    return capi.Engine.batch_config(model, 8, n_problems, keep_history=True)


def _call(eng, fn, a, dev):
    """One call of the raw library; dev: the good arguments on the device, for the two device forms."""
    L, h = eng.L, eng.h
    cfg = _config(a["model"], a["n_problems"])
    shape = (C.byref(cfg), LENGTHS.ctypes.data_as(P32), PARTICLES.ctypes.data_as(P32))
    d = {key: None if a[key] is None else capi._dptr(dev[key]) for key in ("means", "trans", "sigmas", "obs")}
    if fn == "begin_problems":
        return L.cpprob_hip_batch_begin_problems(h, *shape, a["obs"].ctypes.data_as(PD), 2, _p(a["means"]), _p(a["trans"]))
    if fn == "begin_problems_scaled":
        return L.cpprob_hip_batch_begin_problems_scaled(h, *shape, a["obs"].ctypes.data_as(PD), 2, _p(a["means"]), _p(a["trans"]), _p(a["sigmas"]))
    if fn == "begin_online":
        return L.cpprob_hip_batch_begin_online(h, *shape, 2, _p(a["means"]), _p(a["trans"]), SEEDS.ctypes.data_as(P64))
    if fn == "begin_online_scaled":
        return L.cpprob_hip_batch_begin_online_scaled(h, *shape, 2, _p(a["means"]), _p(a["trans"]), _p(a["sigmas"]), SEEDS.ctypes.data_as(P64))
    if fn == "retable":
        return L.cpprob_hip_batch_retable(h, _p(a["means"]), _p(a["trans"]), _p(a["obs"]), a["n_obs"])
    if fn == "retable_scaled":
        return L.cpprob_hip_batch_retable_scaled(h, _p(a["means"]), _p(a["trans"]), _p(a["sigmas"]), _p(a["obs"]), a["n_obs"])
    if fn == "retable_device":
        return L.cpprob_hip_batch_retable_device(h, d["means"], d["trans"], d["obs"], a["n_obs"])
    if fn == "retable_scaled_device":
        return L.cpprob_hip_batch_retable_scaled_device(h, d["means"], d["trans"], d["sigmas"], d["obs"], a["n_obs"])
    if fn == "online_tables":
        return L.cpprob_hip_batch_online_tables(h, _p(a["means"]), _p(a["trans"]))
    assert fn == "online_tables_scaled", fn
    return L.cpprob_hip_batch_online_tables_scaled(h, _p(a["means"]), _p(a["trans"]), _p(a["sigmas"]))


def _error(eng):
    return eng.L.cpprob_hip_last_error(eng.h).decode()


def _good(eng, fn, dev):
    assert _call(eng, fn, _arguments("good"), dev) == 0, (fn, _error(eng))


def _advance(eng, dT):
    at = [0, 3]                                               # where each problem's observes begin in OBS
    done = eng.lengths
    flat = np.concatenate([OBS[at[b] + done[b]:at[b] + done[b] + dT[b]] for b in range(2)])
    assert eng.L.cpprob_hip_batch_advance(eng.h, dT.ctypes.data_as(P32), flat.ctypes.data, 1) == 0, _error(eng)
    eng.lengths = done + dT


def _establish(eng, state, dev):
    """Brings the context into the state, with the good arguments."""
    eng.lengths = np.zeros(2, np.uint32)
    if state == "uniform":
        eng.set_hmm(MEANS[0], TRANS[0])
        obs = np.array([OBS[:3], [OBS[3], OBS[4], 0.25]])
        cfg = _config()
        assert eng.L.cpprob_hip_batch_begin(eng.h, C.byref(cfg), obs.ctypes.data_as(PD), 3) == 0, _error(eng)
    elif state == "hmm3":
        cfg = _config(cp.MODEL_HMM3)
        assert eng.L.cpprob_hip_batch_begin_problems(eng.h, C.byref(cfg), LENGTHS.ctypes.data_as(P32), PARTICLES.ctypes.data_as(P32), OBS.ctypes.data_as(PD), 0, None, None) == 0, _error(eng)
    elif state != "none":
        _good(eng, {"unit": "begin_problems", "scaled": "begin_problems_scaled", "online unit": "begin_online", "online scaled": "begin_online_scaled"}[state], dev)
        if state.startswith("online"):
            _advance(eng, FIRST)


def _results(eng, state):
    """What the begun batch returns: the summaries, the statistics, the ESS and the resampling flags of every step."""
    sums = (capi.Summary * 2)()
    stats, ess, res = np.zeros((2, 3, 3 if state == "hmm3" else 8)), np.zeros((2, 3)), np.zeros((2, 3), np.int32)
    assert eng.L.cpprob_hip_batch_results(eng.h, sums, stats.ctypes.data, stats.size, ess.ctypes.data, res.ctypes.data) == 0, _error(eng)
    return [np.array([[getattr(s, f) for f, _ in capi.Summary._fields_] for s in sums]), stats, ess, res]


def _run(eng, state):
    """The state's batch run with the fixed seeds (an online batch: as it stands after its advances)."""
    if not state.startswith("online"):
        assert eng.L.cpprob_hip_batch_run(eng.h, SEEDS.ctypes.data_as(P64)) == 0, _error(eng)
    return _results(eng, state)


def _equal(x, y):
    return len(x) == len(y) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(x, y))


@pytest.fixture(scope="module")
def dev():
    return {"means": devmem.dtensor(MEANS), "trans": devmem.dtensor(TRANS), "sigmas": devmem.dtensor(SIGMAS), "obs": devmem.dtensor(OBS)}


@pytest.fixture(scope="module")
def reference(dev):
    """What each begun state computes when nothing is refused in between; an online state's after its first advance and after both."""
    eng = cp.Engine(0)
    out = {}
    for state in STATES[2:6]:
        _establish(eng, state, dev)
        out[state] = _run(eng, state)
        if state.startswith("online"):
            _advance(eng, REST)
            out[state + ", advanced"] = _run(eng, state)
    eng.close()
    for a, b in (("unit", "scaled"), ("online unit", "online scaled"), ("online unit", "online unit, advanced")):
        assert not _equal(out[a], out[b]), (a, b)             # (the comparisons below tell the states apart)
    return out


@pytest.mark.parametrize("state", STATES)
def test_every_answer_is_the_tabled_one_and_a_refusal_changes_nothing(state, dev, reference):
    eng = cp.Engine(0)
    try:
        _establish(eng, state, dev)
        if state == "none":
            assert (eng.L.cpprob_hip_batch_run(eng.h, SEEDS.ctypes.data_as(P64)), _error(eng)) == NOT_RUN
        else:
            before = _run(eng, state)
            assert state not in reference or _equal(before, reference[state])
        calls = [(fn, defect, TABLE[fn][state] if isinstance(TABLE[fn][state], tuple) else TABLE[fn][state][defect]) for fn in TABLE for defect in DEFECTS[fn]]
        # the refusals, every one of them before any call that succeeds (no re-table has staged the observes yet)
        for fn, defect, want in calls:
            if want != OK:
                got = (_call(eng, fn, _arguments(defect), dev), _error(eng))
                print("%-22s %-14s %-24s %r" % (fn, state, defect, got))
                assert got == want, (fn, state, defect)
        if state == "none":
            assert (eng.L.cpprob_hip_batch_run(eng.h, SEEDS.ctypes.data_as(P64)), _error(eng)) == NOT_RUN
        else:
            assert _equal(_results(eng, state), before), "the results read differ after the refusals"
            if state.startswith("online"):
                _advance(eng, REST)
                assert _equal(_run(eng, state), reference[state + ", advanced"]), "the online batch advances differently after the refusals"
            else:
                assert _equal(_run(eng, state), before), "the same run differs after the refusals"
        # the calls that succeed: the error text stays, and the batch computes what the state's own begin computes
        for fn, defect, want in calls:
            if want == OK:
                _establish(eng, state, dev)
                text = _error(eng)
                got = (_call(eng, fn, _arguments(defect), dev), _error(eng))
                print("%-22s %-14s %-24s %r" % (fn, state, defect, got[0]))
                assert got == (0, text), (fn, state, defect)
                if fn in BEGINS_AS:
                    eng.lengths = np.zeros(2, np.uint32)
                    if fn.startswith("begin_online"):
                        _advance(eng, FIRST)
                    assert _equal(_run(eng, BEGINS_AS[fn]), reference[BEGINS_AS[fn]]), (fn, state)
                elif fn.startswith("retable"):
                    assert _equal(_run(eng, state), before), (fn, state)
                    if fn in ("retable", "retable_scaled"):        # the observes are staged now: a re-table may leave them out
                        assert _call(eng, fn, _arguments("observes NULL"), dev) == 0, (fn, _error(eng))
                        assert _equal(_run(eng, state), before), (fn, state, "observes NULL")
                else:                                               # (online tables: the same tables, and the batch goes on as it would have)
                    _advance(eng, REST)
                    assert _equal(_run(eng, state), reference[state + ", advanced"]), (fn, state)
    finally:
        eng.close()
