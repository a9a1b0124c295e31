"""Exact references for the variate generators (cpprob/detail/rng.hpp), in plain Python: integers, fractions, mpmath.

A generator is a pure function of a particle's Philox bits, and those are pinned against rocRAND (tests/golden/philox_rocrand.json).
So a draw is checked against the exact inverse CDF at the exact uniform -- nothing here restates a loop or a formula of the kernels:

  uniforms      32-bit: u = w 2^-32;  53-bit: u = B 2^-53, B = lo | (hi >> 11) << 32.  By seed: particle pid takes
                word pid & 3 of block(group pid >> 2), or pair pid & 1 -- words (2(pid & 1), 2(pid & 1) + 1) -- of block(group pid >> 1)
  smallint      a + floor(w R / 2^32), R = b - a + 1
  discrete      #{i < k-1 : u >= C_i / C_k} on the exact values of the weights' doubles
  uniform_real  a + (b - a) u exactly, and the doubles on either side of it
  poisson       the CDF tabulated at 100 digits and held as integers floor(F 2^200): for an integer U, F >= U 2^-200 iff floor(F 2^200) >= U
  normal        sqrt(-2 ln u) sin(pi w), sqrt(-2 ln u) cos(pi w) at 50 digits, u = (v1 + 1) 2^-53, w = (v2 + 1) 2^-52, exact at the quadrant edges
"""
import bisect
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

TWO32, TWO53 = 1 << 32, 1 << 53
FIX = 200                                  # the Poisson CDF in units of 2^-FIX
U53_SHIFT = FIX - 53


# ---- bits -> uniforms --------------------------------------------------------------------------------------------------------------
def bits53(lo, hi):
    return lo | ((hi >> 11) << 32)


def words_of_bits53(b, junk=0):
    """A word pair whose 53 bits are b; `junk` fills the 11 low bits of the high word, which no generator may read."""
    return b & 0xFFFFFFFF, ((b >> 32) << 11) | (junk & 0x7FF)


def normal_v(block):
    x, y, z, w = (int(v) for v in block)
    return x ^ (y << 21), z ^ (w << 21)


def block_of_v(v1, v2):
    """A block whose Box-Muller integers are (v1, v2), each below 2^53."""
    return [v1 & 0x1FFFFF, v1 >> 21, v2 & 0x1FFFFF, v2 >> 21]


@functools.lru_cache(maxsize=None)
def seed_block(O, seed, group, draw):
    """The Philox block of (seed, group, draw) from the oracle's generator, itself pinned against rocRAND."""
    return tuple(int(v) for v in O.draw_block(seed, group, draw))


def seed_words(O, seed, pid0, draw, n):
    """The 32-bit word of particles pid0 .. pid0+n-1 at statement `draw`: word pid & 3 of block(group pid >> 2)."""
    return [seed_block(O, seed, p >> 2, draw)[p & 3] for p in range(pid0, pid0 + n)]


def seed_pairs(O, seed, pid0, draw, n):
    """The (lo, hi) word pair of particles pid0 .. pid0+n-1: words (2(pid & 1), 2(pid & 1) + 1) of block(group pid >> 1)."""
    return [seed_block(O, seed, p >> 1, draw)[2 * (p & 1):2 * (p & 1) + 2] for p in range(pid0, pid0 + n)]


def seed_normal_blocks(O, seed, pid0, draw, n):
    """(block, component) of the normal variate of particles pid0 .. pid0+n-1: component pid & 1 of block(group pid >> 1)."""
    return [(seed_block(O, seed, p >> 1, draw), p & 1) for p in range(pid0, pid0 + n)]


# ---- smallint ----------------------------------------------------------------------------------------------------------------------
def smallint(w, a, b):
    return a + ((w * (b - a + 1)) >> 32)


def smallint_boundary_words(R, n_j=64):
    """Words 0 and 2^32 - 1; for ~n_j values of j spread over the range, the first word that yields j and the word before it; and the
    words midway between neighbouring boundaries."""
    js = sorted({min(R - 1, max(1, (R * i) // n_j)) for i in range(1, n_j + 1)} | {1, R - 1}) if R > 1 else []
    ws = {0, TWO32 - 1}
    for j in js:
        c = -((-j * TWO32) // R)                                     # ceil(j 2^32 / R): the least w with floor(w R / 2^32) >= j
        c1 = -((-(j + 1) * TWO32) // R)
        ws |= {c, c - 1, (c + min(c1, TWO32)) // 2}
    return sorted(w for w in ws if 0 <= w < TWO32)


# ---- discrete ----------------------------------------------------------------------------------------------------------------------
def _cums(weights):
    c, out = Fraction(0), []
    for w in weights:
        c += Fraction(float(w))                                      # the double's exact value
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _discrete_thresholds(weights):
    """ceil(C_i / C_k 2^32), i < k-1: for an integer word, w 2^-32 >= C_i / C_k iff w >= that.  Non-decreasing."""
    C = _cums(weights)
    return [-((-c * TWO32) // C[-1]) for c in C[:-1]]


def discrete(w, weights):
    return bisect.bisect_right(_discrete_thresholds(tuple(weights)), w)


def discrete_boundaries(weights):
    """[(q_i = C_i / C_k 2^32 as a Fraction, exact_in_double)] for i < k-1: exact_in_double says that every partial sum, the total and the
    quotient C_i / C_k are doubles, so that the device's acc / tot IS q_i 2^-32."""
    C = _cums(weights)
    sums_exact = all(Fraction(float(c)) == c for c in C)
    out = []
    for c in C[:-1]:
        r = c / C[-1]
        out.append((r * TWO32, sums_exact and Fraction(float(r)) == r))
    return out


def discrete_row_is_safe(weights):
    """The device compares u = w 2^-32 with acc / tot, which carries a relative error <= k 2^-53: it can disagree with the exact
    comparison only where q_i lies within 2^-20 of an integer without being computed exactly."""
    for q, exact in discrete_boundaries(weights):
        d = abs(q - round(q))
        if d < Fraction(1, 1 << 20) and not (d == 0 and exact):
            return False
    return True


def discrete_boundary_words(weights):
    """Words 0 and 2^32 - 1; at every boundary the least word at or above it and the word before; midpoints between boundaries."""
    qs = sorted({-((-q.numerator) // q.denominator) for q, _ in discrete_boundaries(weights)} | {0, TWO32})
    ws = {0, TWO32 - 1}
    for lo, hi in zip(qs, qs[1:]):
        ws |= {lo, lo - 1, hi, hi - 1, (lo + hi) // 2}
    return sorted(w for w in ws if 0 <= w < TWO32)


# ---- uniform_real ------------------------------------------------------------------------------------------------------------------
def uniform_real(b53, a, b):
    """(below, above): the largest double <= a + (b - a) u and the least double >= it (equal where the value is a double)."""
    x = Fraction(float(a)) + (Fraction(float(b)) - Fraction(float(a))) * Fraction(b53, TWO53)
    f = float(x)                                                     # correctly rounded
    if Fraction(f) == x:
        return f, f
    return (f, math.nextafter(f, math.inf)) if Fraction(f) < x else (math.nextafter(f, -math.inf), f)


# ---- poisson -----------------------------------------------------------------------------------------------------------------------
class PoissonTable:
    """pmf and CDF of Poisson(mean) for the exact value of the double `mean`, by the recurrence p_k = p_{k-1} mean / k at 100 digits.
    F[k] = floor(CDF(k) 2^200) for k <= k_top, the exact quantile of 1 - 2^-54: it lies above every representable u."""

    def __init__(self, mean):
        self.mean = float(mean)
        with mpmath.workdps(100):
            lam = mpmath.mpf(self.mean)
            top = 1 - mpmath.mpf(2) ** -54
            p, F, k = mpmath.exp(-lam), mpmath.mpf(0), 0
            self.pmf, cdf, self.k_top = [], [], None
            mode = int(self.mean)
            while True:
                F += p
                self.pmf.append(p)
                if self.k_top is None:
                    cdf.append(F)
                    if F >= top:
                        self.k_top = k
                # (past k_top, on until a term is below 2^-58 of the mode's: the terms the generator can add are counted from these)
                if self.k_top is not None and k >= mode and p < self.pmf[mode] * mpmath.mpf(2) ** -58:
                    break
                k += 1
                p = p * lam / k
            self.cdf = cdf
            self.F = [int(mpmath.floor(mpmath.ldexp(f, FIX))) for f in cdf]
            pm = self.pmf[mode]
            self.n_below = sum(1 for q in self.pmf[:mode] if q > pm * mpmath.mpf(2) ** -56)
            self.n_above = sum(1 for q in self.pmf[mode + 1:] if q > pm * mpmath.mpf(2) ** -56)

    def quantile_fix(self, U):
        """min{k : CDF(k) >= U 2^-200} for an integer U, capped at k_top."""
        return min(bisect.bisect_left(self.F, U), self.k_top)

    def accept(self, b53, delta_fix):
        """[k_min, k_max]: the exact quantiles at u' in [u - delta, u + delta] (u' >= 0), none above k_top."""
        U = b53 << U53_SHIFT
        return self.quantile_fix(max(0, U - delta_fix)), self.quantile_fix(U + delta_fix)

    def boundary_bits(self, pmf_floor=1e-18):
        """For every k with pmf > pmf_floor: the largest 53-bit u <= CDF(k) and the next u above it."""
        out = set()
        for k, f in enumerate(self.F):
            if self.pmf[k] > pmf_floor:
                b = f >> U53_SHIFT
                out |= {b, b + 1}
        return sorted(b for b in out if 0 <= b < TWO53)

    def interior_bits(self, pmf_floor=2.0 ** -30):
        """Midway between the CDF values on either side of every k with pmf > pmf_floor: one acceptable value."""
        out = []
        for k, f in enumerate(self.F):
            if self.pmf[k] > pmf_floor:
                below = self.F[k - 1] if k else 0
                out.append(((below + f) // 2) >> U53_SHIFT)
        return out


@functools.lru_cache(maxsize=None)
def poisson_table(mean):
    return PoissonTable(mean)


# ---- normal ------------------------------------------------------------------------------------------------------------------------
def _sincospi(w):
    """(sin(pi w), cos(pi w)) for a Fraction w: exact integers at the multiples of 1/2, mpmath elsewhere."""
    if (2 * w).denominator == 1:
        q = int(2 * w) % 4
        return ((0, 1), (1, 0), (0, -1), (-1, 0))[q]
    x = mpmath.pi * mpmath.mpf(w.numerator) / w.denominator
    return mpmath.sin(x), mpmath.cos(x)


def normal(block):
    """(x, y, s) as mpmath numbers (exact ints where sin / cos is 0 or +-1 or s is 0): x = s sin(pi w), y = s cos(pi w)."""
    v1, v2 = normal_v(block)
    with mpmath.workdps(50):
        u = mpmath.mpf(v1 + 1) / TWO53
        s = mpmath.sqrt(-2 * mpmath.log(u)) if v1 + 1 < TWO53 else 0
        sn, cs = _sincospi(Fraction(v2 + 1, 1 << 52))
        return s * sn, s * cs, s


def normal_error_ok(got, ref, rel=3 * 2.0 ** -52):
    """|got - ref| <= rel |ref|, evaluated at 50 digits; an exactly zero reference asks for an exact zero."""
    if ref == 0:
        return got == 0.0
    with mpmath.workdps(50):
        return abs(mpmath.mpf(float(got)) - ref) <= rel * abs(ref)


def as_u32(blocks):
    return np.ascontiguousarray(np.array(blocks, dtype=np.uint64).astype(np.uint32).reshape(-1, 4))
