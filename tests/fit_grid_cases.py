"""Constructed inputs for the fitting kernels (csrc/batch_scale.hpp, batch_retable.hpp, batch_learn*.hpp) where the suite's runs of a
few problems do not reach: table_log, scale_entry's division and scale_sigma's square root across their domains, and batches of so
many problems that the M-step's threads leave the first workgroup and retable_grid_y's share makes a workgroup walk several tiles.
tests/test_fit_grid_cases_host.py proves on the CPU that every input reaches what it claims; tests/test_gpu_batch_fit_domain.py and
tests/test_gpu_batch_fit_grids.py run them on the device.  Nothing here needs a GPU."""
import math

import numpy as np

import retable_ref as R
import scale_ref as S

K = 8
SIGMA_FLOOR = 1e-160
LENGTHS = (1, 31, 32, 33, 64, 65, 70)


# arguments whose mantissas lie just below table_log's fold, for the padding (see log_sigmas)
BELOW_THE_FOLD = [math.ldexp(S.SQRT2 - 2.5e-4 * (i + 1), e) for i, e in enumerate((-500, 3, 700))]


def log_sigmas():
    """[B_log, 8]: sigma = sqrt(x / 2 pi) for every argument x of test_scale_ref_host.ARGS whose sigma the check takes, so that the
    logarithm's argument (2 pi sigma) sigma runs over ARGS up to three roundings; padded to a multiple of 8 with 1.0 -- but for the
    last three places of the padding, which carry BELOW_THE_FOLD: of ARGS' mantissas 9 lie within 1e-3 below the fold and 13 within
    1e-3 above it, and ten on either side are asked for."""
    from test_scale_ref_host import ARGS
    sg = [math.sqrt(x / S.TWO_PI) for x in ARGS]
    sg = [s for s in sg if not S.bad(s)]
    pad = -len(sg) % K
    sg += [1.0] * pad
    if pad >= 4:
        sg[-3:] = [math.sqrt(x / S.TWO_PI) for x in BELOW_THE_FOLD]
    return np.array(sg).reshape(-1, K)


def n_log_sigmas():
    """The sigmas of log_sigmas() that are not padding."""
    from test_scale_ref_host import ARGS
    return sum(1 for x in ARGS if not S.bad(math.sqrt(x / S.TWO_PI)))


# Variances v whose sigma = sqrt(v) has a log_norm that a fused multiply-add changes: found by a seeded search over 1.3 million
# variances (exp(u) / 2 pi, u uniform over +-700, +-40 and +-3) with table_log_fused below, which differs from table_log at one
# argument in some 6000 -- none of log_sigmas()'s 16048 arguments is among them, so without these a device build of table_log with
# contraction left on would pass.  The first differs where the Horner steps are fused alone, the second there and at q = 1 + s p, the
# others at q = 1 + s p alone; no argument was found at which the fusion of e kLn2Lo + r shows.
FUSED_V = [float.fromhex(h) for h in (
    "0x1.d06002cdc5e87p-2", "0x1.dda45169d1df5p-1", "0x1.d5d5e354b5dffp-1", "0x1.97e7e60aac3b1p-4", "0x1.bd2d236aa3483p-4", "0x1.a8b5cba3c834cp-4",
    "0x1.d5fc1c1b02a29p-4", "0x1.f92b7f587c349p-3", "0x1.f7e958c69451fp-5", "0x1.20983e84735f5p-2", "0x1.ec3540b54437dp-7", "0x1.ae0f2bd180c81p-4",
    "0x1.f19b8c49b287cp-3", "0x1.a232de22b2007p-5", "0x1.d155c0fc59e67p-6", "0x1.b1145eb1f7d7fp-3", "0x1.84c17ec5a6b40p-2", "0x1.d167bcbe0cb55p-5",
    "0x1.ecbee239bf448p-1", "0x1.9f2a8d091bf48p-2", "0x1.d511f06e2b1e4p-4", "0x1.dc0416a824b28p-6", "0x1.1965c1514657ep+1", "0x1.c2e4e7b5f32bap-1",
    "0x1.0496dac3669dbp-3", "0x1.a87fd416fc530p+2", "0x1.a92ad268def3cp-3", "0x1.b5277c6a79a33p-3", "0x1.becee84eac4a6p-5", "0x1.ee6d6f175cadfp-5",
    "0x1.e48e13fa60a95p+0", "0x1.c7e201295bc65p-6", "0x1.a8b6d3801b791p-3", "0x1.04861f106c553p-3", "0x1.a0998ed4f128fp-3", "0x1.bbb15e22fa7fcp+0",
    "0x1.f980eaac1c4afp-3", "0x1.e03e9aa106971p-2", "0x1.a39afc166e028p-5", "0x1.c258e0a161c48p-5", "0x1.7c05f01db37cfp-7", "0x1.e51afe820641bp-3",
    "0x1.db80d636c1bf7p-3", "0x1.02935918ae3cbp-4", "0x1.d2cbcbda7d5d0p-3", "0x1.b300c7fecf389p-4", "0x1.7c4d1262d32c4p-3", "0x1.d923b331b0820p-4",
    "0x1.a57dfc4f98b29p-6", "0x1.9f064f661ce60p-4", "0x1.f98395a736c87p-4", "0x1.0aafb00d2796dp-3", "0x1.b4f64218f757ep-5", "0x1.b18b34c04c1c2p-3",
    "0x1.ec4116c2dd6dcp-4", "0x1.b660a9e33f9dbp-3", "0x1.a2146d0c9e077p-4", "0x1.8974d30bb983ap-5", "0x1.039ec2b6858fcp-2", "0x1.fc0896f9ef475p-2",
    "0x1.ce473ec8ff9f3p-3", "0x1.e5a86284e2f87p-4", "0x1.d7f8d40d2fda3p-1", "0x1.db20afdd473c0p-4")]


def _fma(a, b, c):
    """The correctly rounded a b + c (exact rational arithmetic, rounded once)."""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def table_log_fused(x, horner=True, q=True, lo=True):
    """scale_ref.table_log with the named product-and-sum pairs fused, as a compiler that contracts would form them (e kLn2Hi is exact,
    so fusing hi + lo changes nothing)."""
    import struct
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    e = ((u >> 52) & 0x7FF) - 1023
    m = struct.unpack("<d", struct.pack("<Q", (u & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000))[0]
    if m >= S.SQRT2:
        m, e = m * 0.5, e + 1
    f = (m - 1.0) / (m + 1.0)
    s = f * f
    p = S.COEF[0]
    for c in S.COEF[1:]:
        p = _fma(p, s, c) if horner else p * s + c
    qq = _fma(s, p, 1.0) if q else 1.0 + s * p
    r = (f + f) * qq
    ed = float(e)
    low = _fma(ed, S.LN2_LO, r) if lo else ed * S.LN2_LO + r
    return ed * S.LN2_HI + low


def fused_case():
    """(variances [8, 8], sigmas [8, 8]) of FUSED_V: sigma = sqrt(v), the M-step's own statement."""
    v = np.array(FUSED_V).reshape(-1, K)
    return v, np.sqrt(v)


def division_case(B=None, seed=20261021):
    """(y [B], means [B, 8], sigmas [B, 8]): one observe a problem, every mean 0.0 (so y - mean is y, exactly), sigma a random mantissa
    at an exponent -20 .. 20, y a random sign and mantissa at an exponent that puts every |y / sigma| of its problem in 2^10 .. 2^60.
    The quotient's square is then so far above log_norm that a quotient one ulp off changes the row (row_from_quotient)."""
    B = log_sigmas().shape[0] if B is None else int(B)
    rng = np.random.default_rng(seed)
    es = rng.integers(-20, 21, (B, K))
    sigmas = np.ldexp(1.0 + rng.random((B, K)), es)
    # |y| = my 2^ey, sigma = ms 2^es, my / ms in (1/2, 2): the quotient's exponent is ey - es - 1 or ey - es
    lo, hi = 11 + es.max(axis=1), 59 + es.min(axis=1)
    assert np.all(lo <= hi)
    ey = lo + (rng.random(B) * (hi - lo + 1)).astype(np.int64)
    y = np.ldexp(1.0 + rng.random(B), ey) * np.where(rng.random(B) < 0.5, -1.0, 1.0)
    return y, np.zeros((B, K)), sigmas


def row_from_quotient(q, log_norm):
    """scale_entry's statements behind the division, elementwise."""
    r = np.asarray(q, np.float64) * np.asarray(q, np.float64)
    r = r + np.asarray(log_norm, np.float64)
    return r * np.float64(-0.5)


def mstep_records(seed=20261022):
    """(records [B_log, 88], means [B_log, 8], trans [B_log, 8, 8], sigmas [B_log, 8]) for k = 8 and the floor SIGMA_FLOOR: occ_y = 0
    (the new mean is 0 and v = occ_yy / occ), occ a random mantissa in [1, 2), occ_yy = the double of log_sigmas()^2 occ -- v runs over
    log_sigmas()^2 up to two roundings, sigma' = sqrt(v) over log_sigmas().  The seven padding states carry the other branches: v = 0
    (the floor, whose 2 pi sigma^2 is subnormal: refused), an infinite v (an infinite sigma': refused), a state without mass, a NaN
    occ_yy (the floor).  The transition counts are random, with a row without mass in every seventh problem."""
    sg = log_sigmas()
    B = sg.shape[0]
    rng = np.random.default_rng(seed)
    rec = np.zeros((B, R.RECORD))
    rec[:, :64] = rng.uniform(0.0, 3.0, (B, 64))
    rec[::7, 8:16] = 0.0
    occ = 1.0 + rng.random((B, K))
    with np.errstate(all="ignore"):
        occ_yy = (sg * sg) * occ
    pad = B * K - n_log_sigmas()
    assert pad == 7
    occ_yy[-1, 1], occ_yy[-1, 2], occ[-1, 3], occ_yy[-1, 4] = 0.0, np.inf, 0.0, np.nan
    rec[:, 64:72], rec[:, 80:88] = occ, occ_yy
    means = rng.uniform(-3.0, 3.0, (B, K))
    trans = rng.uniform(0.05, 1.0, (B, K, K))
    sigmas = rng.uniform(0.3, 2.5, (B, K))
    return rec, means, trans, sigmas


def many_lengths(B, seed=20261023):
    """[B] lengths drawn from LENGTHS, each of them present; the last problem is one of the longest."""
    rng = np.random.default_rng(seed)
    Ts = rng.choice(LENGTHS, int(B))
    Ts[:len(LENGTHS)] = LENGTHS
    Ts[-1] = max(LENGTHS)
    return [int(T) for T in Ts]


def many_problems(B, k=K, seed=20261023):
    """(lengths [B], observes, tables A, tables B) of a batch of B problems: the lengths of many_lengths, observes and tables
    (means, transition, sigmas) as tests/test_gpu_batch_scale.py draws them."""
    from test_gpu_batch_scale import _observes, _tables
    Ts = many_lengths(B, seed)
    return Ts, _observes(Ts, k, seed + 1), _tables(B, k, seed + 2), _tables(B, k, seed + 3)


def tiles_walked(T, B):
    """For a launch of retable_grid_y(T, B) workgroups a problem: the tiles of 32 rows workgroup y walks, for every y."""
    gy = R.grid_y(T, B)
    trips = (T + R.ROWS_PER_TRIP - 1) // R.ROWS_PER_TRIP
    return [list(range(y, trips, gy)) for y in range(gy)]


LEARN_CAP, LEARN_FIRST = 75, 5
LEARN_SECOND = (70, 0, 31, 32, 33, 65, 1, 64)


def learn_schedule(B):
    """Two advances of an online batch of B streams of capacity LEARN_CAP: LEARN_FIRST observes each, then LEARN_SECOND's counts
    in turn -- the new rows start at the unaligned row 5, some problems sit the second advance out, the longest piece is 70."""
    second = [LEARN_SECOND[b % len(LEARN_SECOND)] for b in range(int(B))]
    second[-1] = max(LEARN_SECOND)
    return [[LEARN_FIRST] * int(B), second]
