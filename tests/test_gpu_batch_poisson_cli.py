"""Poisson emissions through cpprob_main --batch_tables_file ... --poisson_emissions (cpprob::gpu::HmmTable::emission,
Options::rate_floor): every line of the tables file carries [rates] [transition] [observes], the observes counts; with --em_iterations N
-- the host loop, --em_on_device and --tie_tables -- the fitted rates are printed where the means are and are, with the transition rows and
the evidences, the ones cpprob_amd.hmm_table_em(emission="poisson") returns for the same input, to the 17 significant digits printed; the
plain batch and --stream_chunk print the Python route's evidences; the flag is refused by name where it has nothing to act on."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def _list(text):
    return np.array([float(v) for v in text.split()])


def _fitted(line, k):
    assert line.startswith("[") and line.endswith("]"), line
    m, t = line[1:-1].split("] [")
    return _list(m), _list(t).reshape(k, k)


def test_cli_prints_the_rates_the_python_route_returns(engine, tmp_path):
    n, seed, k = 300, 12, 3
    rates = np.array([[0.5, 4.0, 12.0], [1.0, 3.0, 9.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [40, 17]
    obs = [rng.poisson(rates[b][rng.integers(0, 3, T)]).astype(np.float64) for b, T in enumerate(Ts)]

    def write(name, r, t):
        (tmp_path / name).write_text("".join("%s %s %s\n" % (_numbers(r[b]), _numbers(t[b]), _numbers(obs[b])) for b in range(2)))
    write("tables.txt", rates, trans)
    base = [MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt",
            "--poisson_emissions"]
    seeds = np.arange(seed, seed + 2, dtype=np.uint64)

    def run(cmd, lines_expected=4):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.strip().splitlines()
        assert len(lines) == lines_expected, p.stdout
        return lines
    # particle EM: the host loop, --em_on_device, another floor
    for extra, floor in (([], 1e-6), (["--em_on_device"], 1e-6), (["--rate_floor", "2.5"], 2.5)):
        m, t, ev = cp.hmm_table_em(engine, obs, rates, trans, n, seeds, 2, emission="poisson", rate_floor=floor)
        lines = run(base + ["--em_iterations", "2"] + extra)
        for b in range(2):
            assert _list(lines[b])[0] == ev[-1, b], (extra, b)
            got = _fitted(lines[2 + b], k)
            assert np.array_equal(got[0], m[-1, b]) and np.array_equal(got[1], t[-1, b]), (extra, b)
        assert not np.array_equal(m[-1], rates) and (floor < 1.0 or np.any(m[-1] == 2.5))
    # tied: both recordings under one table
    tied_r, tied_t = np.tile(rates[0], (2, 1)), np.tile(trans[0], (2, 1, 1))
    write("tied.txt", tied_r, tied_t)
    tied = [a if a != "tables.txt" else "tied.txt" for a in base]
    m, t, ev = cp.hmm_table_em(engine, obs, tied_r, tied_t, n, seeds, 2, emission="poisson", groups=np.zeros(2, np.int64))
    for extra in ([], ["--em_on_device"]):
        lines = run(tied + ["--em_iterations", "2", "--tie_tables"] + extra)
        assert lines[2] == lines[3]
        for b in range(2):
            assert _list(lines[b])[0] == ev[-1, b], (extra, b)
            got = _fitted(lines[2 + b], k)
            assert np.array_equal(got[0], m[-1, b]) and np.array_equal(got[1], t[-1, b]), (extra, b)
    # the plain batch and the stream: the evidences of the Python route
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(rates, trans), emission="poisson")
    engine.batch_run(seeds)
    want = [s["log_evidence"] for s in engine.batch_results()[0]]
    assert [_list(x)[0] for x in run(base, 2)] == want
    assert [_list(x)[0] for x in run(base + ["--stream_chunk", "7"], 2)] == want
    # refusals, by name
    for extra, words in ((["--emission_scales"], ("--poisson_emissions", "--emission_scales")),
                         (["--stream_chunk", "7", "--online_em"], ("--online_em", "Poisson")),
                         (["--em_iterations", "2", "--rate_floor", "0"], ("rate_floor",))):
        q = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert q.returncode != 0 and all(w in q.stderr for w in words), (extra, q.stderr)
    q = subprocess.run([a for a in base if a not in ("--batch_tables_file", "tables.txt")] + ["--model", "hmm16", "--observes", "[1 2 3]"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--poisson_emissions" in q.stderr and "--batch_tables_file" in q.stderr
