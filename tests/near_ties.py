"""Near-tie cases of the prefix-count (table-weight) resamplers of the built-in HMM (MODEL_HMM3, every-step schedule).

Every ancestor of that form is decided by comparing two rounded doubles: the systematic comb's fma(C_k, N/W, -u0) against an output
index j, the stratified comb's H = C_k * (N/W) against F + u_F, the multinomial threshold tau_s = fma(v_s, B_w+1 - B_w, B_w) against a
particle's CDF value C_k -- and, over shards, against a rank's mass bound P_b (exchange_cut_kernel).  A kernel that rounds one of these
differently from the oracle decides differently only when the two sides lie within an ulp or so, which random inputs almost never hit.
This module constructs inputs that put a chosen comparison exactly on a tie, or one ulp to either side of it.

The state counts of generation t depend only on the seed and on y_0 .. y_{t-1}; y_t enters the resampling that follows generation t only
through the weight table e = exp(ll - max ll) (oracle: orc_hmm_weight_table).  Stepping y_t one ulp at a time moves the CDF values by a
few ulps, so a bisection of y_t over its bit pattern walks (A - B) across zero a few ulps at a time, and the ulps around the crossing hold
the gaps -1, 0 and +1.  Every quantity comes from the oracle (table CDF, weight table, Philox uniforms, thresholds); only fma, which
Python 3.10 lacks, is evaluated exactly with fractions.Fraction (float(Fraction) is correctly rounded).

A case is SHARP when some plausible rounding change of its one decision -- one side moved by an ulp, a non-strict compare for a strict
one, a contracted mul+add (the multinomial width fma((w + 1), unit, -B_w), the stratified fma(C, inv, -F)), an unfused systematic
fma -- changes an ancestor of the oracle's resampling, or (the cut rows) the rank a threshold is sourced from.  check_case() re-proves
that from the oracle; `python tests/near_ties.py` searches the cases and writes tests/golden/near_ties.json."""
import json
import math
import os
import struct
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "near_ties.json")
TILE = 1024
RESAMPLE_DRAW_BASE2 = (1 << 40) + (1 << 39)
ROWS = ("systematic", "stratified", "multinomial", "cut")
RESAMPLER = {"systematic": O.RESAMPLE_SYSTEMATIC, "stratified": O.RESAMPLE_STRATIFIED, "multinomial": O.RESAMPLE_MULTINOMIAL,
             "cut": O.RESAMPLE_MULTINOMIAL}


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def okey(x):
    """Order-preserving integer of a double (adjacent doubles differ by 1)."""
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)


def ofloat(i):
    b = i if i >= 0 else (-i) | (1 << 63)
    return struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0]


def gap(a, b):
    """a - b in ulps (the number of doubles between them, signed)."""
    return okey(a) - okey(b)


class Generation:
    """Generation t = len(y_prefix) of an every-step SMC run of MODEL_HMM3: its states, their prefix counts, the resampling's step."""

    def __init__(self, seed, n, y_prefix, resampler):
        self.seed, self.n, self.y_prefix, self.rs = int(seed), int(n), [float(y) for y in y_prefix], resampler
        self.t = len(self.y_prefix)
        self.step = self.t + 1
        self.x = O.smc(O.MODEL_HMM3, self.y_prefix + [0.0], self.n, self.seed, resampler, 2.0)["hist"][self.t].copy()
        self.c0 = np.cumsum(self.x == 0)
        self.c1 = np.cumsum(self.x == 1)
        self.k_levels = int(O.lib().orc_strata_levels(self.n))
        self._tau = None

    def counts(self, k):
        """Inclusive prefix counts of the states 0, 1, 2 through particle k."""
        c0, c1 = int(self.c0[k]), int(self.c1[k])
        return np.array([c0, c1, k + 1 - c0 - c1], np.uint64)

    def cdf(self, k, e):
        return O.table_cdf(self.counts(k), e)

    def strata(self):
        if self._tau is None:
            self._tau = O.strata_thresholds_table(1.0, self.seed, self.step, self.n)[1]
        return self._tau

    def v(self, s):
        r = O.draw_block(self.seed, s >> 1, RESAMPLE_DRAW_BASE2 + self.step)
        lo, hi = (r[2], r[3]) if s & 1 else (r[0], r[1])
        return float(O.lib().orc_u01_53(int(lo), int(hi)))

    def oracle_ancestors(self, y):
        e = O.hmm_weight_table(y)[0]
        if self.rs == O.RESAMPLE_SYSTEMATIC:
            return O.resample_table_systematic(self.x, e, self.seed, self.step)
        if self.rs == O.RESAMPLE_STRATIFIED:
            return O.resample_table_stratified(self.x, e, self.seed, self.step)
        return O.resample_table_multinomial(self.x, e, self.seed, self.step)


def decision(row, g, y, k, out):
    """The comparison that decides whether particle k (or, for `cut`, the rank that ends with particle k) owns output `out`:
    dict(A, B, pred, alt={name: pred}) -- pred as the oracle rounds it, alt under the alternative roundings."""
    e = O.hmm_weight_table(y)[0]
    W = g.cdf(g.n - 1, e)
    C = g.cdf(k, e)
    up, dn = math.nextafter(C, math.inf), math.nextafter(C, -math.inf)
    c0, c1, c2 = (float(c) for c in g.counts(k))
    # the CDF value in another order of the canonical fma(c2, e2, fma(c1, e1, c0 * e0)): unfused, and nested the other way round
    cdf_alt = {"cdf-unfused": c0 * e[0] + c1 * e[1] + c2 * e[2], "cdf-reversed": fma(c0, e[0], fma(c1, e[1], c2 * e[2]))}
    if row == "systematic":
        N = float(g.n)
        inv = N / W
        u0 = O.resample_u0(g.seed, g.step)
        j = float(out)
        z = fma(C, inv, -u0)                                 # G_k = ceil(z): particle k owns beyond output j iff G_k > j iff z > j
        alt = {"C+1ulp": fma(up, inv, -u0) > j, "C-1ulp": fma(dn, inv, -u0) > j, "unfused": C * inv - u0 > j, "non-strict": z >= j}
        alt.update({name: fma(Ca, inv, -u0) > j for name, Ca in cdf_alt.items()})
        return dict(A=z, B=j, pred=z > j, alt=alt)
    if row == "stratified":
        N = float(g.n)
        inv = N / W
        F = float(out)
        u = O.stratified_u(g.seed, g.step, out)
        H = C * inv                                          # A_k = F + [u_F < H - F]: k owns beyond output F iff u_F < H - F
        alt = {"C+1ulp": u < up * inv - F, "C-1ulp": u < dn * inv - F, "contracted": u < fma(C, inv, -F), "non-strict": u <= H - F}
        alt.update({name: u < Ca * inv - F for name, Ca in cdf_alt.items()})
        return dict(A=H, B=F + u, pred=u < H - F, alt=alt)
    # multinomial / cut: tau_s = fma(v_s, B_w+1 - B_w, B_w), B_w = w * (W 2^-k); k owns beyond output s iff C_k > tau_s
    unit = math.ldexp(W, -g.k_levels)
    w = int(g.strata()[out])
    v = g.v(out)
    b0, b1 = w * unit, (w + 1) * unit
    tau = fma(v, b1 - b0, b0)
    tau_c = fma(v, float(Fraction(w + 1) * Fraction(unit) - Fraction(b0)), b0)       # hipcc's contraction of (w + 1) * unit - B_w
    alt = {"tau+1ulp": C > math.nextafter(tau, math.inf), "tau-1ulp": C > math.nextafter(tau, -math.inf), "contracted": C > tau_c, "non-strict": C >= tau}
    alt.update({name: Ca > tau for name, Ca in cdf_alt.items()})
    return dict(A=C, B=tau, pred=C > tau, w=w, alt=alt)


def pick_output(row, g, y, k):
    e = O.hmm_weight_table(y)[0]
    W = g.cdf(g.n - 1, e)
    C = g.cdf(k, e)
    if row == "systematic":
        return int(round(C * (g.n / W) - O.resample_u0(g.seed, g.step)))
    if row == "stratified":
        return int(math.floor(C * (g.n / W)))
    tau = O.strata_thresholds_table(W, g.seed, g.step, g.n)[0]
    return int(np.argmin(np.abs(tau - C)))


def check_case(case, g=None):
    """Re-prove a case from the oracle.  Returns dict(gap, sharp=[alternatives that change an ancestor / a source rank]); raises
    AssertionError where the emulated decision disagrees with the oracle's own resampling."""
    row, k, out = case["row"], case["k"], case["out"]
    y = float.fromhex(case["obs"][case["gen"]])
    if g is None:
        g = Generation(case["seed"], case["n"], [float.fromhex(h) for h in case["obs"][:case["gen"]]], RESAMPLER[row])
    d = decision(row, g, y, k, out)
    flips = [name for name, p in d["alt"].items() if p != d["pred"]]
    if row == "cut":
        # the oracle over shards: ranks [.., k] and [k + 1, ..] -- which of the two sources output `out`
        e = O.hmm_weight_table(y)[0]
        W = g.cdf(g.n - 1, e)
        tau = O.strata_thresholds_table(W, g.seed, g.step, g.n)[0]
        assert tau[out] == d["B"], "threshold emulation differs from the oracle"
        tot = g.counts(g.n - 1)
        left = O.resample_table_multinomial_shard(g.x[:k + 1], e, g.seed, g.step, np.zeros(3, np.uint64), tot, False, g.n)
        right = O.resample_table_multinomial_shard(g.x[k + 1:], e, g.seed, g.step, g.counts(k), tot, True, g.n)
        assert (left[out] >= 0) == d["pred"] and (right[out] >= 0) == (not d["pred"]), "oracle's shard split disagrees with the emulated decision"
        sharp = flips                                                      # (a flip IS a change of the source rank)
    else:
        anc = g.oracle_ancestors(y)
        a = int(anc[out])
        assert (a <= k) == d["pred"], "oracle's ancestor disagrees with the emulated decision"
        # flipping k's decision changes anc[out] unless an earlier particle already owns it
        sharp = flips if (not d["pred"] or a == k) else []
    return dict(gap=gap(d["A"], d["B"]), sharp=sharp)


# ---- the search -----------------------------------------------------------------------------------------------------------------

def _sign(row, g, y, k, out):
    d = decision(row, g, y, k, out)
    return (d["A"] > d["B"]) - (d["A"] < d["B"])


def search(row, g, y0, k, want=(-1, 0, 1), span=40):
    """Bisect y over its bit pattern until (A - B) changes sign, then look `span` ulps of y to either side for the gaps in `want`
    whose cases are sharp.  Returns {gap: y}."""
    out = pick_output(row, g, y0, k)
    s0 = _sign(row, g, y0, k, out)
    lo = hi = None
    for delta in (1e-4, 1e-3, 1e-2, 3e-2, 0.1, 0.3):
        for y1 in (y0 - delta, y0 + delta):
            if _sign(row, g, y1, k, out) == -s0:
                lo, hi = okey(y0), okey(y1)
                break
        if lo is not None:
            break
    if lo is None:
        return out, {}
    if lo > hi:
        lo, hi = hi, lo
    slo = _sign(row, g, ofloat(lo), k, out)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        sm = _sign(row, g, ofloat(mid), k, out)
        if sm == 0:
            lo = hi = mid
            break
        if sm == slo:
            lo = mid
        else:
            hi = mid
    found = {}
    base = dict(row=row, seed=g.seed, n=g.n, gen=g.t, k=k, out=out)
    for i in sorted(range(lo - span, hi + span + 1), key=lambda i: abs(i - lo)):
        y = ofloat(i)
        d = decision(row, g, y, k, out)
        gp = gap(d["A"], d["B"])
        if gp not in want or gp in found:
            continue
        if all(p == d["pred"] for p in d["alt"].values()):
            continue
        if row == "cut" and gp >= 0 and d["alt"]["contracted"] == d["pred"]:
            continue                                     # (the tie and +1 ulp cut cases: those the unpinned cut kernel decides differently)
        case = dict(base, obs=[h.hex() for h in g.y_prefix] + [y.hex()])
        r = check_case(case, g)
        if r["sharp"]:
            found[gp] = y
        if len(found) == len(want):
            break
    return out, found


POSITIONS = ("interior", "tile_first", "tile_last", "shard_end")


def _particle(position, n, i):
    m = ((n // TILE) // 3 + 7 * i) % (n // TILE - 2) + 1
    return {"interior": m * TILE + 517, "tile_first": m * TILE, "tile_last": m * TILE + 1023, "shard_end": m * TILE + 389 + 2 * i}[position]


def shard_layout(case, ranks):
    """Shard sizes for a loopback group of `ranks` ranks.  `cut` and `shard_end` cases end a shard at particle k, so that the tied
    quantity is a rank's mass bound P_b; the others begin shards on tile boundaries, so that k keeps its place in its tile."""
    n, k = case["n"], case["k"]
    if case["row"] == "cut" or case["position"] == "shard_end":
        first = [k + 1]
    else:
        b = TILE * max(1, (k // TILE) // 2)
        first = [b]
    rest = n - sum(first)
    m = ranks - len(first)
    cuts = [rest * (i + 1) // m for i in range(m)]
    sizes = first + [cuts[0]] + [cuts[i] - cuts[i - 1] for i in range(1, m)]
    if case["row"] == "cut" and m >= 2:
        sizes[1] += 3; sizes[2] -= 3                     # ragged later boundaries too
    assert sum(sizes) == n and min(sizes) > 0
    return sizes


def build_cases(verbose=True):
    cases = []
    y_later = 0.35                                       # y_0 of the later-generation cases
    plan = [("systematic", 100000, 11), ("stratified", 100000, 12), ("multinomial", 150001, 13), ("cut", 150001, 14)]
    for row, n, seed in plan:
        for gen in (0, 1):
            prefix = [] if gen == 0 else [y_later]
            g = Generation(seed + 100 * gen, n, prefix, RESAMPLER[row])
            need, placed = {-1, 0, 1}, set()
            i = 0
            while (need or len(placed) < len(POSITIONS)) and i < 32:
                position = POSITIONS[i % len(POSITIONS)]
                i += 1
                if position in placed and not need:
                    continue
                k = _particle(position, n, i)
                out, found = search(row, g, 0.2 + 0.05 * (i % 8), k, span=40 if need != {-1} else 400)
                for gp, y in sorted(found.items()):
                    if gp not in need and position in placed:
                        continue
                    ranks = 2 + len(cases) % 7
                    case = dict(row=row, seed=g.seed, n=n, gen=gen, k=k, out=out, position=position, gap=gp,
                                obs=[h.hex() for h in prefix] + [y.hex(), (0.1).hex()])
                    case["shards"] = shard_layout(case, ranks)
                    case["sharp"] = check_case(case, g)["sharp"]
                    cases.append(case)
                    need.discard(gp)
                    placed.add(position)
                    if verbose:
                        print(row, "gen", gen, position, "k", k, "out", out, "gap", gp, "y", y.hex(), "sharp", case["sharp"], flush=True)
            if need and verbose:
                print("!!", row, "gen", gen, "missing gaps", sorted(need), flush=True)
    return cases


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


if __name__ == "__main__":
    cases = build_cases()
    with open(GOLDEN, "w") as f:
        json.dump({"about": "near-tie cases of the prefix-count resamplers (tests/near_ties.py)", "cases": cases}, f, indent=1)
        f.write("\n")
    print("wrote %d cases to %s" % (len(cases), GOLDEN))
