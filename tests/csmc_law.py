"""The invariance experiment of the conditional SMC run, shared by tests/test_csmc_ref_host.py (on the CPU reference) and
tests/test_gpu_batch_csmc_law.py (one batch on the device): a k = 2, T = 3 table HMM whose posterior over the 8 state paths is
enumerated exactly; N reference paths are drawn from it, every one takes ONE sweep "conditional run with n = 2 particles, then one
backward-simulated trajectory" under its own seed, and the N trajectories must again be draws from the posterior.  The same sweep on
an unconditional run's masses is not: its law differs from the posterior by the filter's error at n = 2.

The exact law is that of the device's own integers: the transition masses P[s][s'] 2^-32 of the 32-bit thresholds and a uniform
initial state (smallint_from_word halves the 32-bit words exactly for k = 2); the emission constants cancel."""
import functools
import itertools

import numpy as np

import backward_ref as R
import csmc_ref as CS
from oracle import oracle as O

K, T, N, N_PARTICLES = 2, 3, 16384, 2
MEANS = [-1.0, 1.0]
TRANS = [[0.9, 0.1], [0.2, 0.8]]
OBS = [1.2, -0.8, 1.5]
PATHS = list(itertools.product(range(K), repeat=T))       # path j = (x_0, x_1, x_2), x_0 the slowest index


def tables():
    """(ll [T][k], thr [k][k-1], P [k][k] integers) of the model."""
    return R.log_likelihoods(OBS, MEANS), R.thresholds(TRANS), R.transition_masses(TRANS)


@functools.lru_cache(maxsize=None)
def exact_law():
    """p[j] of PATHS[j], float64 [8]."""
    ll, _, P = tables()
    p = np.array([(1.0 / K) * np.exp(ll[0][x[0]]) * np.prod([P[x[t - 1]][x[t]] / 2.0**32 * np.exp(ll[t][x[t]]) for t in range(1, T)]) for x in PATHS])
    return p / p.sum()


def bound():
    """5 sigma of a cell's frequency among N iid draws of the exact law."""
    p = exact_law()
    return 5.0 * np.sqrt(p * (1.0 - p) / N)


@functools.lru_cache(maxsize=None)
def reference_paths():
    """int32 [N, T]: iid draws of the exact law (a fixed generator)."""
    rng = np.random.default_rng(20231)
    return np.array(PATHS, np.int32)[rng.choice(len(PATHS), N, p=exact_law())]


def histogram(traj):
    """Frequencies of the 8 paths among trajectories [N, T]."""
    code = np.asarray(traj, np.int64) @ (K ** np.arange(T - 1, -1, -1))
    return np.bincount(code, minlength=K**T) / float(len(traj))


@functools.lru_cache(maxsize=None)
def conditional_histogram():
    """The CPU reference's: problem i has seed i and reference path reference_paths()[i]."""
    ll, thr, P = tables()
    ref = reference_paths()
    out = np.zeros((N, T), np.int32)
    for i in range(N):
        out[i] = R.trajectories(CS.masses(ll, thr, i, N_PARTICLES, ref[i]), P, i, 1)[:, 0]
    return histogram(out)


@functools.lru_cache(maxsize=None)
def unconditional_histogram():
    """The same sweep on the masses of the oracle's unconditional run (systematic resampling, n = 2) under seed i."""
    ll, _, P = tables()
    O.set_hmm(MEANS, TRANS)
    out = np.zeros((N, T), np.int32)
    for i in range(N):
        hist = O.smc(O.MODEL_HMM_TABLE, np.array(OBS), N_PARTICLES, i)["hist"]
        out[i] = R.trajectories(R.filtering_masses(hist, ll), P, i, 1)[:, 0]
    return histogram(out)
