"""Particle EM through cpprob_main --batch_tables_file ... --em_iterations N (cpprob::gpu::hmm_table_fit): the fitted tables it prints
after the usual output are cpprob_amd.hmm_table_em's, and the usual output is the last run's."""
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


def test_cli_fits_the_tables_hmm_table_em_fits(engine, tmp_path):
    n, seed, iters = 700, 12, 3
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [40, 17]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    p = subprocess.run([MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed),
                        "--batch_tables_file", "tables.txt", "--em_iterations", str(iters)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 4, p.stdout
    m_hist, t_hist, ev = cp.hmm_table_em(engine, obs, means, trans, n, np.arange(seed, seed + 2, dtype=np.uint64), iters)
    for b in range(2):
        usual = _list(lines[b])
        assert usual[0] == ev[-1, b] and usual.size == 1 + 3 * Ts[b], b
        assert lines[2 + b].startswith("[") and lines[2 + b].endswith("]"), lines[2 + b]
        got_m, got_t = lines[2 + b][1:-1].split("] [")
        # (printed with 17 significant digits: the doubles themselves)
        assert np.array_equal(_list(got_m), m_hist[-1, b]), b
        assert np.array_equal(_list(got_t).reshape(3, 3), t_hist[-1, b]), b
    assert not np.array_equal(m_hist[-1], means)
    # the iterations are refused where a batch is fed in pieces
    q = subprocess.run([MAIN, "--model_folder", str(tmp_path), "--smc", "--n_samples", str(n), "--batch_tables_file", "tables.txt", "--em_iterations", "2",
                        "--stream_chunk", "4"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--stream_chunk" in q.stderr
