"""The cases of the variate-generator tests and their checks against tests/variate_ref.py, written once for two back ends: the CPU
oracle's functions (tests/test_variates_host.py) and the device's (tests/test_gpu_variates.py).  A back end has

    from_bits(which, params, blocks)            blocks: uint32 [n, 4] -> (out0, out1) float64 [n] (out1: normal's second output)
    by_seed(which, params, seed, pid0, draw, n) -> the draws of particles pid0 .. pid0+n-1 through the shipped draw entries

Every condition that concerns the reference alone (a row has no boundary within rounding reach, a point has one acceptable value,
delta <= 2^-40) is asserted here too, so it is checked wherever the cases run.
"""
import functools
import math

import numpy as np

import variate_ref as R

SMALLINT, DISCRETE, UNIFORM_REAL, POISSON, NORMAL = 0, 1, 2, 3, 4
POISSON_MAX_MEAN = 1.0e4                      # CPPROB_HIP_POISSON_MAX_MEAN

N_SEED = 20000
PID0S = (0, 1, 2, 3, 2 ** 32 - 2)             # odd and unaligned offsets; particle ids that cross 32 bits
PID0S_WIDE = (2 ** 33 - 2, 2 ** 34 - 2)       # ... and the group id itself: pid >> 1 and pid >> 2 cross 32 bits (a short window each)
N_WIDE = 64


def _blocks_word0(words):
    """Blocks whose word 0 is given; the other three hold bits a 32-bit generator must not read."""
    return R.as_u32([[w, 0xFFFFFFFF ^ w, 0xA5A5A5A5, (w * 2654435761) & 0xFFFFFFFF] for w in words])


def _blocks_bits53(bits):
    return R.as_u32([list(R.words_of_bits53(b, junk=0x7FF * (i & 1))) + [0xDEADBEEF, (b * 40503) & 0xFFFFFFFF] for i, b in enumerate(bits)])


def _fail(kind, bad, n):
    assert not bad, "%s: %d of %d wrong; first: %s" % (kind, len(bad), n, "; ".join(bad[:6]))


# ---- smallint: pure integer arithmetic, delta = 0 ------------------------------------------------------------------------------------
SMALLINT_RANGES = (1, 2, 3, 7, 255, 256, 257, 65535, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32)
SMALLINT_LOWS = (0, 5, -7, -2 ** 31)
SMALLINT_SEED = ((0, 2), (-7, 250), (-2 ** 31, 2 ** 31 - 1))


def check_smallint_bits(be):
    for rng in SMALLINT_RANGES:
        words = R.smallint_boundary_words(rng)
        for a in SMALLINT_LOWS:
            b = a + rng - 1
            want = np.array([R.smallint(w, a, b) for w in words], dtype=np.float64)
            got, _ = be.from_bits(SMALLINT, (a, b), _blocks_word0(words))
            assert want.min() >= a and want.max() <= b
            bad = ["w=%#x: %d, exact %d" % (w, g, e) for w, g, e in zip(words, got, want) if g != e]
            _fail("smallint(%d, %d)" % (a, b), bad, len(words))


def check_smallint_seed(be, O):
    for j, (a, b) in enumerate(SMALLINT_SEED):
        for pid0, n in [(p, N_SEED) for p in (PID0S if j == 0 else PID0S[1:2])] + [(p, N_WIDE) for p in PID0S_WIDE]:
            want = np.array([R.smallint(w, a, b) for w in R.seed_words(O, 42, pid0, 5, n)], dtype=np.int64)
            got = np.asarray(be.by_seed(SMALLINT, (a, b), 42, pid0, 5, n), dtype=np.int64)
            assert np.array_equal(got, want), "smallint(%d, %d) by seed, pid0 = %d: %d of %d differ" % (a, b, pid0, int(np.sum(got != want)), n)


# ---- discrete: delta = 0 on rows without a boundary in rounding reach --------------------------------------------------------------
DISCRETE_ROWS = (
    [1.0],                                                   # k = 1 .. 8
    [0.5, 0.5], [0.25, 0.5, 0.25], [1.0, 2.0, 1.0, 4.0],     # dyadic: exact in floating point, boundaries ON words
    [0.5, 0.25, 0.5],
    [0.0, 1.0], [1.0, 0.0], [0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 0.0, 3.0, 0.0, 5.0, 0.0],   # zeros: leading, middle, trailing
    [3.0, 1.0, 2.0, 2.0], [10.0, 20.0, 30.0, 40.0, 50.0],    # unnormalised
    [0.1] * 7, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0],
    [1.0, 1e-17, 2.0], [1e-300] * 3,                         # spanning 1 and 1e-17; tiny throughout
    [0.1, 0.5, 0.4], [0.2, 0.2, 0.6], [0.15, 0.15, 0.7],     # the rows of test_draws_match_oracle
)
DISCRETE_SEED = ([0.1, 0.5, 0.4], [0.0, 0.0, 3.0, 0.0, 5.0, 0.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])


def check_discrete_rows_are_safe():
    assert {len(r) for r in DISCRETE_ROWS} == set(range(1, 9))
    for row in DISCRETE_ROWS:
        assert R.discrete_row_is_safe(row), "row %s has a boundary within 2^-20 of a word that floating point does not compute exactly" % row


def check_discrete_bits(be):
    check_discrete_rows_are_safe()
    for row in DISCRETE_ROWS:
        words = R.discrete_boundary_words(row)
        want = np.array([R.discrete(w, row) for w in words], dtype=np.float64)
        assert all(row[int(i)] > 0 for i in want), "the reference drew a zero-weight index"
        got, _ = be.from_bits(DISCRETE, row, _blocks_word0(words))
        bad = ["w=%#x: %d, exact %d" % (w, g, e) for w, g, e in zip(words, got, want) if g != e]
        _fail("discrete%s" % row, bad, len(words))


def check_discrete_seed(be, O):
    for j, row in enumerate(DISCRETE_SEED):
        for pid0, n in [(p, N_SEED) for p in (PID0S if j == 0 else PID0S[3:4])] + [(p, N_WIDE) for p in PID0S_WIDE]:
            want = np.array([R.discrete(w, row) for w in R.seed_words(O, 9, pid0, 7, n)], dtype=np.int64)
            got = np.asarray(be.by_seed(DISCRETE, row, 9, pid0, 7, n), dtype=np.int64)
            assert np.array_equal(got, want), "discrete%s by seed, pid0 = %d: %d of %d differ" % (row, pid0, int(np.sum(got != want)), n)


# ---- uniform_real: one of the two doubles next to the exact value, and in [a, b) ---------------------------------------------------
UNIFORM_PAIRS = ((0.0, 1.0), (1.0, 2.0), (-3.0, 5.0), (1e6, 1e6 + 1), (-1.0, -1.0 + 2.0 ** -40), (-1e300, 1e300), (0.75, 0.75))
UNIFORM_BITS = (0, 1, 2 ** 53 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 53 - 2, 0x15555555555555, 0x0AAAAAAAAAAAAB, 3, 2 ** 21)
UNIFORM_SEED = ((-3.0, 5.0), (1.0, 2.0))


def _uniform_bad(bits, got, a, b):
    bad = []
    for u, g in zip(bits, got):
        lo, hi = R.uniform_real(u, a, b)
        g = float(g)
        if not ((g == lo or g == hi) and (a <= g < b if a < b else g == a)):
            bad.append("u=%#x/2^53: %r, exact value between %r and %r" % (u, g, lo, hi))
    return bad


def check_uniform_real_bits(be):
    for a, b in UNIFORM_PAIRS:
        got, _ = be.from_bits(UNIFORM_REAL, (a, b), _blocks_bits53(UNIFORM_BITS))
        _fail("uniform_real(%r, %r)" % (a, b), _uniform_bad(UNIFORM_BITS, got, a, b), len(UNIFORM_BITS))


def check_uniform_real_seed(be, O):
    for j, (a, b) in enumerate(UNIFORM_SEED):
        for pid0, n in [(p, N_SEED) for p in (PID0S if j == 0 else PID0S[1:2])] + [(p, N_WIDE) for p in PID0S_WIDE]:
            bits = [R.bits53(lo, hi) for lo, hi in R.seed_pairs(O, 1, pid0, 2, n)]
            got = be.by_seed(UNIFORM_REAL, (a, b), 1, pid0, 2, n)
            _fail("uniform_real(%r, %r) by seed, pid0 = %d" % (a, b, pid0), _uniform_bad(bits, got, a, b), n)


# ---- poisson -------------------------------------------------------------------------------------------------------------------------
POISSON_MEANS = (0.0, 2.0 ** -60, 0.3, 1.0, 3.7, 4.0, 25.0, 100.0, 500.0, 700.0, 708.0, 740.0, 745.0, 746.0, 1000.0, 1.0e4)
POISSON_SEED = (25.0, 0.3, 4.0, 745.0, 1.0e4)


def poisson_delta(tab):
    """The error bound of the generator's CDF, in the uniform: |C_k / S - F(k)| <= delta(mean) = (2 W + 8 sqrt(mean) + 16) 2^-53.

    Derived from the arithmetic of poisson_from_u (cpprob/detail/rng.hpp), eps = 2^-53 the unit roundoff, m = floor(mean), tau_j =
    pmf(j) / pmf(m), Z = sum tau_j = 1 / pmf(m):
      * terms.  t_m = 1; each step away from the mode is one division and one product, so t_j = tau_j (1 + th_j), |th_j| <= 2 |j - m| eps.
        Weighted by tau_j / Z = pmf(j) they sum to at most 2 eps E|X - m| <= 2 eps (sqrt(mean) + 1)      (E|X - mean| <= sd, |mean - m| < 1).
      * sums.  A cumulative weight C_k is reached by at most W additions or subtractions of partial sums that never exceed S, each rounded
        once: W eps.  A term is added only while it changes its sum, t > ulp(sum) / 2 > 2^-54 sum, and the sums are >= 1/2 from the
        first term on (t_m = 1, t_{m-1} = m / mean > 1/2), so only terms with tau_j > 2^-56 are ever added: n_below of them under the mode
        and n_above over it, COUNTED ON THE EXACT pmf.  Upwards the walk makes n_below + n_above + 1 additions, downwards n_below additions
        and at most n_below subtractions: W = n_below + max(n_below, n_above + 1).
      * dropped tails.  The first term not added is <= eps sum, and the terms beyond it fall at least as fast as the geometric series of its
        ratio rho: mean / (mean - s) times it below the mode, (k + 1) / (k + 1 - mean) above.  It is i steps from the mode with
        1 - i (i + 1) / (2 mean) <= tau <= 2^-45 (the sums stay below 256 for mean <= 10^4), so i >= max(1, sqrt(2 mean) - 1.01), and both
        factors are <= 2 + sqrt(mean): 2 (2 + sqrt(mean)) eps for the two tails.
      Together C_k / Z and S / Z are within eta = (W + 4 sqrt(mean) + 6) eps of F(k) and of 1; the quotient C_k / S is within 2 eta (1 + eta),
      and the threshold T = fl(u S) adds eps: delta = (2 W + 8 sqrt(mean) + 13) eps + second-order terms < (2 W + 8 sqrt(mean) + 16) eps.
    A fused multiply-add in place of a product and a sum only removes a rounding.  The bound is a condition: the callers assert
    delta <= 2^-40 for every tested mean (at mean 10^4: W = 1762, delta = 2^-40.92)."""
    w = tab.n_below + max(tab.n_below, tab.n_above + 1)
    return (2 * w + 8 * math.sqrt(tab.mean) + 16) * 2.0 ** -53


def _delta_fix(tab):
    d = poisson_delta(tab)
    assert d <= 2.0 ** -40, "delta(%r) = 2^%.2f" % (tab.mean, math.log2(d))
    return int(math.ceil(d * 2.0 ** 60)) << (R.FIX - 60)             # rounded up to a multiple of 2^-60


def _poisson_bad(tab, dfix, bits, got, unique=False):
    bad = []
    for u, g in zip(bits, got):
        lo, hi = tab.accept(u, dfix)
        if unique:
            assert lo == hi, "mean %r, u = %#x / 2^53: the reference accepts %d .. %d" % (tab.mean, u, lo, hi)
        if not (lo <= g <= hi and g == int(g)):
            bad.append("u=%#x/2^53: %r, exact quantile %s (k_top %d)" % (u, g, lo if lo == hi else "%d..%d" % (lo, hi), tab.k_top))
    return bad


def check_poisson_bits(be, means=POISSON_MEANS):
    for mean in means:
        assert mean <= POISSON_MAX_MEAN
        tab = R.poisson_table(mean)
        dfix = _delta_fix(tab)
        edge = sorted({0, 1, 2 ** 53 - 1} | set(tab.boundary_bits()))
        mid = tab.interior_bits()
        got, _ = be.from_bits(POISSON, (mean,), _blocks_bits53(edge + mid))
        bad = _poisson_bad(tab, dfix, edge, got[:len(edge)]) + _poisson_bad(tab, dfix, mid, got[len(edge):], unique=True)
        _fail("poisson(%r)" % mean, bad, len(edge) + len(mid))


def check_poisson_seed(be, O):
    for j, mean in enumerate(POISSON_SEED):
        tab = R.poisson_table(mean)
        dfix = _delta_fix(tab)
        for pid0, n in [(p, N_SEED) for p in (PID0S if j == 0 else PID0S[3:4])] + [(p, N_WIDE) for p in PID0S_WIDE]:
            bits = [R.bits53(lo, hi) for lo, hi in R.seed_pairs(O, 5, pid0, 1, n)]
            got = be.by_seed(POISSON, (mean,), 5, pid0, 1, n)
            _fail("poisson(%r) by seed, pid0 = %d" % (mean, pid0), _poisson_bad(tab, dfix, bits, got, unique=True), n)


# ---- normal: |got - ref| <= 3 2^-52 |ref| ------------------------------------------------------------------------------------------------
# (log01 <= 1 ulp, halved by a correctly rounded sqrt (+0.5); sincospi02 <= 1.05; one product (+0.5): 2.55 ulp, each <= 2^-52 relative --
#  the bounds tests/test_gpu_blocks.py asserts on the device's elementary functions)
NORMAL_V1 = sorted({0, 1, 2 ** 53 - 1} | {2 ** j - 1 for j in range(1, 54)} | {2 ** j - 2 for j in (2, 10, 21, 22, 32, 33, 52, 53)})
NORMAL_V2 = sorted({0, 2 ** 53 - 1} | {k * 2 ** 50 - 1 + d for k in range(1, 9) for d in (-1, 0, 1) if k * 2 ** 50 - 1 + d < 2 ** 53})
NORMAL_SEED = 3


@functools.lru_cache(maxsize=None)
def _normal_ref(block):
    return R.normal(block)


def _normal_bad(blocks, x, y):
    bad = []
    for blk, gx, gy in zip(blocks, x, y):
        rx, ry, _ = _normal_ref(tuple(blk))
        for name, g, r in (("x", gx, rx), ("y", gy, ry)):
            if g is not None and not R.normal_error_ok(g, r):
                bad.append("v=(%#x, %#x) %s: %r, exact %s" % (R.normal_v(blk) + (name, float(g), r)))
    return bad


def check_normal_bits(be, O):
    blocks = [R.block_of_v(v1, v2) for v1 in NORMAL_V1 for v2 in NORMAL_V2]
    x, y = be.from_bits(NORMAL, (), R.as_u32(blocks))
    _fail("normal, constructed bits", _normal_bad(blocks, x, y), 2 * len(blocks))
    # where sin or cos is +-1 the output is +-s: the four quadrant edges of one v1 agree exactly in magnitude, with the signs of the circle
    at = {(v1, v2): (float(gx), float(gy)) for (v1, v2), gx, gy in zip(((v1, v2) for v1 in NORMAL_V1 for v2 in NORMAL_V2), x, y)}
    for v1 in NORMAL_V1:
        s = at[(v1, 2 * 2 ** 50 - 1)][0]                              # w = 1/2: x = s
        assert s >= 0.0 and (s > 0.0) == (v1 < 2 ** 53 - 1)
        assert at[(v1, 2 * 2 ** 50 - 1)][1] == 0.0
        assert at[(v1, 4 * 2 ** 50 - 1)] == (0.0, -s)                 # w = 1
        assert at[(v1, 6 * 2 ** 50 - 1)] == (-s, 0.0)                 # w = 3/2
        assert at[(v1, 8 * 2 ** 50 - 1)] == (0.0, s)                  # w = 2
    blocks = [list(R.seed_block(O, NORMAL_SEED, g, 0)) for g in range(N_SEED)]      # 20000 random blocks: those of particles 0 .. 39999
    x, y = be.from_bits(NORMAL, (), R.as_u32(blocks))
    _fail("normal, random blocks", _normal_bad(blocks, x, y), 2 * len(blocks))


def check_normal_seed(be, O):
    for pid0, n in [(p, N_SEED) for p in PID0S] + [(p, N_WIDE) for p in PID0S_WIDE]:
        got = be.by_seed(NORMAL, (0.0, 1.0), NORMAL_SEED, pid0, 0, n)          # mean 0, sigma 1: 0 + 1 z is z
        blocks, comp = zip(*R.seed_normal_blocks(O, NORMAL_SEED, pid0, 0, n))
        x = [None if c else g for c, g in zip(comp, got)]
        y = [g if c else None for c, g in zip(comp, got)]
        _fail("normal by seed, pid0 = %d" % pid0, _normal_bad(blocks, x, y), n)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
REFUSED = (
    (SMALLINT, (0, 2 ** 31)), (SMALLINT, (-2 ** 31 - 1, 0)), (SMALLINT, (2 ** 40, 2 ** 40 + 1)),
    (DISCRETE, [0.5, -0.1, 0.6]), (DISCRETE, [0.5, float("nan")]), (DISCRETE, [1.0, float("inf")]), (DISCRETE, [0.0, 0.0, 0.0]),
    (DISCRETE, [1e308, 1e308]),
    (POISSON, (math.nextafter(POISSON_MAX_MEAN, math.inf),)), (POISSON, (1e300,)), (POISSON, (float("nan"),)), (POISSON, (-1.0,)),
)
