"""Near-tie cases at the batched kernel's own partition edges (csrc/batch_smc.hpp), built with tests/near_ties.py.

The batched kernel lays a problem's particles out as passes of 1024 (one LDS pass), wavefronts of 256 particles inside a pass, and runs
of four particles a lane; the comb of each lane starts from the exclusive prefix at its first particle.  Every case here puts the
systematic or stratified decision of one particle k exactly on a tie or one ulp from it (generation 0 or 1, n = 8192), with k at the
first / last particle of a lane's run, of a wavefront and of an LDS pass, or in the interior.  check_case() re-proves each case sharp.
All cases have T = 3 observes (the observes after the tied step only shape later generations), so they run as problems of ONE batch.
`python tests/near_ties_batch.py` searches the cases and writes tests/golden/near_ties_batch.json."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import near_ties as NT  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "near_ties_batch.json")
N = 8192
T = 3
# particle k of each partition edge: pass p, wave w (256 particles), lane l (4 particles)
POSITIONS = {
    "lane_first": 3 * 1024 + 4 * 37,
    "lane_last": 3 * 1024 + 4 * 37 + 3,
    "wave_first": 5 * 1024 + 256,
    "wave_last": 5 * 1024 + 511,
    "pass_first": 6 * 1024,
    "pass_last": 2 * 1024 - 1,
    "interior": 4 * 1024 + 517,
}


def build_cases(verbose=True):
    cases = []
    for row, seed in (("systematic", 21), ("stratified", 22)):
        for gen in (0, 1):
            prefix = [] if gen == 0 else [0.35]
            g = NT.Generation(seed + 100 * gen, N, prefix, NT.RESAMPLER[row])
            for position, k in POSITIONS.items():
                for attempt in range(6):
                    out, found = NT.search(row, g, 0.2 + 0.07 * attempt, k)
                    if found:
                        break
                for gp, y in sorted(found.items()):
                    obs = prefix + [y] + [0.1] * (T - 1 - gen)
                    case = dict(row=row, seed=g.seed, n=N, gen=gen, k=k, out=out, position=position, gap=gp, obs=[v.hex() for v in obs])
                    case["sharp"] = NT.check_case(case, g)["sharp"]
                    cases.append(case)
                    if verbose:
                        print(row, "gen", gen, position, "k", k, "out", out, "gap", gp, "sharp", case["sharp"], flush=True)
    return cases


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


if __name__ == "__main__":
    cases = build_cases()
    with open(GOLDEN, "w") as f:
        json.dump({"about": "near-tie cases at the batched kernel's partition edges (tests/near_ties_batch.py)", "cases": cases}, f, indent=1)
        f.write("\n")
    print("wrote %d cases to %s" % (len(cases), GOLDEN))
