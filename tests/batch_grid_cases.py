"""The batches tests/test_gpu_batch_decode_grid.py and tests/test_gpu_batch_forecast_grid.py share: shapes at which the loops of
csrc/batch_decode.hpp, csrc/batch_forecast.hpp and csrc/batch_suffstats.hpp run more than once.  No test lives here."""
import numpy as np

import backward_ref as R
import cpprob_amd as cp
from oracle import exact
from test_gpu_batch_smooth_lag import _seeds, _table_observes, _tables

K_WAVE, K_WAVES, K_THREADS, K_TILE = 64, 4, 256, 1024
DECODE_TRACE_GRID_MAX, PREDICTIVE_GRID_MAX = 4096, 4096          # kDecodeTraceGridMax, kPredictiveGridMax

# The long ragged batch: HMM_TABLE, k = 5, a table a problem (table 1 with a zero transition entry).  B = 11 is three workgroups of
# the forward and statistics kernels, the last with three problems; the lengths sit on both sides of the traceback's 64-word chunks,
# and problem 0 owes more rows than one trip of the predictive kernel (16384) holds.
LONG_K = 5
LONG_TS = [16500, 1, 63, 64, 65, 128, 129, 600, 2, 300, 23]
LONG_NS = [5, 1, 70, 3, 300, 64, 65, 8, 1025, 16, 100]
SHORT = list(range(1, 11))                                       # the problems of at most 600 steps: the one-trip twin

# The online stream: 150 observes fed as 63 + 1 + 1 + 63 + 1 + 21, so that the forward pass resumes at 63, 64, 65, 128 and 129.
# Problem 1 is never fed; problem 4's capacity ends its stream at 128.
ONLINE_K = 5
ONLINE_CAPS = [150, 9, 151, 150, 128, 160]
ONLINE_NS = [70, 3, 5, 300, 64, 1025]
ONLINE_CUT = [63, 1, 1, 63, 1, 21]
ONLINE_UNFED = 1


def long_case():
    """(model, Ts, ns, means [B, k], trans [B, k, k], observes, seeds)."""
    means, trans = _tables(LONG_K, len(LONG_TS), 83)
    return cp.MODEL_HMM_TABLE, list(LONG_TS), list(LONG_NS), means, trans, _table_observes(means, LONG_TS, 83), _seeds(len(LONG_TS), 89)


def sub_case(case, idx):
    """The problems `idx` of a case, as a batch of their own."""
    model, Ts, ns, means, trans, obs, seeds = case
    return model, [Ts[b] for b in idx], [ns[b] for b in idx], means[idx], trans[idx], [obs[b] for b in idx], seeds[idx]


def hmm3_case():
    """A uniform batch under the model's one table: B = 9 (three workgroups of the forward kernel, the last with one problem),
    T = 130 (three chunks of the traceback), n = 70."""
    B, T = 9, 130
    return (cp.MODEL_HMM3, [T] * B, [70] * B, np.array([exact.HMM_MEAN] * B), np.array([exact.HMM_T] * B),
            [exact.simulate_hmm(T, 7000 + b) for b in range(B)], _seeds(B, 97))


def online_case():
    """(means, trans, observes by capacity, seeds) of the online stream."""
    B = len(ONLINE_CAPS)
    means, trans = _tables(ONLINE_K, B, 101)
    return means, trans, _table_observes(means, ONLINE_CAPS, 101), _seeds(B, 103)


def online_lengths():
    """The lengths [B] after each advance of ONLINE_CUT."""
    out, lens = [], [0] * len(ONLINE_CAPS)
    for dT in ONLINE_CUT:
        lens = [L if b == ONLINE_UNFED else min(L + dT, ONLINE_CAPS[b]) for b, L in enumerate(lens)]
        out.append(list(lens))
    return out


def begin(engine, case, **kw):
    """Begins and runs a case: a uniform HMM3 batch through batch_begin, anything else as described problems."""
    model, Ts, ns, means, trans, obs, seeds = case
    if model == cp.MODEL_HMM3:
        engine.batch_begin(model, np.array(obs), ns[0], **kw)
    else:
        engine.batch_begin_problems(model, obs, ns, tables=(means, trans), **kw)
    engine.batch_run(seeds)


def masses(engine, case, b):
    """(m, ll) of problem b from the rows its run left."""
    vals, _, logw = engine.batch_store(b)
    ll = R.log_likelihoods(case[5][b], case[3][b])
    assert np.all(logw == np.array(ll[-1])[vals[-1]]), "problem %d: restated log-likelihoods differ from the run's table" % b
    return R.filtering_masses(vals, ll), ll


def kept_masses(engine, b, k):
    """m of problem b from the table a keep_masses batch keeps."""
    return [[int(x) for x in row[:k]] for row in engine.batch_masses(b)]


def pass_grid(engine, what, forward=None, trace=None, forecast=None, predictive=None):
    """Asserts the grids of engine's last decode / forecast / predictive call (cpprob_hip_batch_pass_grid) where a value is given."""
    got = dict(zip(("forward", "trace", "forecast", "predictive"), engine.batch_pass_grid()))
    print("%s: forward gridDim.x %d, trace gridDim.y %d, forecast gridDim.y %d, predictive gridDim.y %d" % (
        what, got["forward"], got["trace"], got["forecast"], got["predictive"]))
    for name, want in (("forward", forward), ("trace", trace), ("forecast", forecast), ("predictive", predictive)):
        assert want is None or got[name] == want, "%s: %s grid %d, expected %d" % (what, name, got[name], want)
    return got


def trace_grid(lens, lag, frm=None):
    """gridDim.y of a fixed-lag traceback over the lengths `lens`: row 0 and the rows of 256 lane items."""
    fr = [0] * len(lens) if frm is None else frm
    items = max([L - 1 - f - lag for L, f in zip(lens, fr)] + [0])
    return 1 + min(-(-items // K_THREADS), DECODE_TRACE_GRID_MAX), items


def predictive_grid(lens, frm=None):
    """(gridDim.y, trips of the problem that owes most, rows it owes) of a predictive call."""
    fr = [0] * len(lens) if frm is None else frm
    owed = max(L + 1 - f for L, f in zip(lens, fr))
    gy = min(-(-owed // K_WAVES), PREDICTIVE_GRID_MAX)
    return gy, -(-owed // (gy * K_WAVES)), owed


def chunks(L, first=0):
    """The 64-word chunks row 0 of the traceback stages for steps first .. L - 1."""
    return -(-(L - first) // K_WAVE) if L > first else 0
