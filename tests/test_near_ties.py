"""The near-tie cases of tests/golden/near_ties.json (tests/near_ties.py) are SHARP: each puts one integer-deciding comparison of
the prefix-count resamplers exactly on a tie or one ulp from it, and some plausible rounding change of that comparison -- a side moved
by an ulp, a non-strict compare, a contracted mul+add, another order of the CDF's fmas -- changes an ancestor of the oracle's
resampling, or the rank that sources a threshold.  Re-proved from the oracle on every run, so the fixture cannot go stale; the GPU
side (tests/test_gpu_near_ties.py) runs the same cases against the oracle and the one-GPU run."""
import collections

import pytest

import near_ties as NT

CASES = NT.load_cases()


@pytest.fixture(scope="module")
def proofs():
    gens, out = {}, []
    for c in CASES:
        key = (c["row"], c["seed"], c["n"], tuple(c["obs"][:c["gen"]]))
        if key not in gens:
            gens[key] = NT.Generation(c["seed"], c["n"], [float.fromhex(h) for h in key[3]], NT.RESAMPLER[c["row"]])
        out.append(NT.check_case(c, gens[key]))
    return out


def test_every_case_is_a_sharp_near_tie(proofs):
    for c, p in zip(CASES, proofs):
        assert p["gap"] == c["gap"] and c["gap"] in (-1, 0, 1), c
        assert p["sharp"], ("no rounding change alters this case's outcome", c)
        assert p["sharp"] == c["sharp"], c


def test_every_row_holds_ties_and_one_ulp_gaps_in_two_generations(proofs):
    table = collections.defaultdict(collections.Counter)
    for c in CASES:
        table[c["row"]][c["gap"]] += 1
    print("\nsharp near-tie cases per row (gap in ulps: count):")
    for row in NT.ROWS:
        print("  %-12s tie %d  +1 ulp %d  -1 ulp %d" % (row, table[row][0], table[row][1], table[row][-1]))
        assert all(table[row][gp] >= 1 for gp in (-1, 0, 1)) and sum(table[row].values()) >= 3, row
        assert {c["gen"] for c in CASES if c["row"] == row} == {0, 1}, row
        assert len({c["position"] for c in CASES if c["row"] == row}) >= 3, row


def test_cut_cases_separate_the_contracted_width_from_the_oracle(proofs):
    """The tie and +1 ulp cut cases: the threshold a contracted width fma((w + 1), unit, -B_w) yields lies on the other side of the
    rank bound P_b from the oracle's -- the rank that sources the output changes.  Their shards end at particle k, so P_b is the tie."""
    n_contracted = collections.Counter()
    for c, p in zip(CASES, proofs):
        if c["row"] != "cut":
            continue
        assert sum(c["shards"][:1]) == c["k"] + 1 and sum(c["shards"]) == c["n"], c
        if c["gap"] >= 0:
            assert "contracted" in p["sharp"], c
            n_contracted[c["gap"]] += 1
    assert n_contracted[0] >= 1 and n_contracted[1] >= 1


def test_layouts_are_loopback_groups_of_two_to_eight_ranks():
    for c in CASES:
        assert 2 <= len(c["shards"]) <= 8 and min(c["shards"]) > 0 and sum(c["shards"]) == c["n"], c
        assert 100_000 <= c["n"] <= 400_000 and 2 <= len(c["obs"]) <= 4
