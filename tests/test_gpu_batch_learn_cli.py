"""Online EM through cpprob_main --batch_tables_file ... --stream_chunk K --online_em (cpprob::gpu::Options::learn_tables,
cpprob::gpu::HmmTableStream): the tables it prints after the usual output, in the format --em_iterations prints them, are the ones
cpprob_amd.hmm_table_online_em returns for the same input -- with the history and, --filtering_only --keep_masses, from the masses
alone; without a stream, or with neither history nor masses, the flag is refused by name."""
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


def test_cli_prints_the_tables_the_driver_returns(engine, tmp_path):
    n, seed, k, chunk = 300, 12, 3, 4
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [40, 17]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    base = [MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt"]
    seeds = np.arange(seed, seed + 2, dtype=np.uint64)
    for extra, kw in ((["--em_burn_in", "8"], dict(t_min=8, keep_history=True)),
                      (["--em_burn_in", "8", "--em_step_exponent", "0.75", "--filtering_only", "--keep_masses"], dict(t_min=8, step_exponent=0.75, keep_history=False)),
                      ([], dict(t_min=20, keep_history=True))):
        m, t, st, sums = cp.hmm_table_online_em(engine, obs, (means, trans), n, seeds, chunk, **kw)
        assert not st.any() and not np.array_equal(m[-1], means)
        p = subprocess.run(base + ["--stream_chunk", str(chunk), "--online_em"] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 4, p.stdout
        for b in range(2):
            assert _list(lines[b])[0] == sums[b]["log_evidence"], (extra, b)
            line = lines[2 + b]
            assert line.startswith("[") and line.endswith("]"), line
            got_m, got_t = line[1:-1].split("] [")
            # (printed with 17 significant digits: the doubles themselves)
            assert np.array_equal(_list(got_m), m[-1, b]) and np.array_equal(_list(got_t).reshape(k, k), t[-1, b]), (extra, b)
    # no stream; neither history nor masses: refused by name
    q = subprocess.run(base + ["--online_em"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--online_em" in q.stderr and "--stream_chunk" in q.stderr
    q = subprocess.run(base + ["--online_em", "--stream_chunk", "4", "--filtering_only"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--online_em" in q.stderr and "--keep_masses" in q.stderr
