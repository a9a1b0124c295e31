"""Running statistics through cpprob_main --batch_tables_file ... --stream_chunk K --running_stats
(cpprob::gpu::Options::running_stats, cpprob::gpu::HmmTableStream): the line a problem it prints after the usual output is
Engine.batch_online_stats' record of the whole stream -- the same doubles whatever the chunk, with the history and, --filtering_only
--keep_masses, from the masses alone; without a stream, or with neither history nor masses, the flag is refused by name."""
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


def test_cli_prints_the_engines_running_records(engine, tmp_path):
    n, seed, k = 300, 12, 3
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [40, 17]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    base = [MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt"]
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, Ts, n, np.arange(seed, seed + 2, dtype=np.uint64), tables=(means, trans))
    engine.batch_advance(obs)
    want = engine.batch_online_stats(obs)
    ev = [s["log_evidence"] for s in engine.batch_results()[0]]
    assert np.abs(want["occ"].sum(axis=1) - np.array(Ts)).max() <= 1e-9
    for extra in (["--stream_chunk", "7"], ["--stream_chunk", "1"], ["--stream_chunk", "64", "--filtering_only", "--keep_masses"]):
        p = subprocess.run(base + ["--running_stats"] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 4, p.stdout
        for b in range(2):
            assert _list(lines[b])[0] == ev[b], (extra, b)
            line = lines[2 + b]
            assert line.startswith("[") and line.endswith("]"), line
            xi, occ, occ_y, occ_yy = line[1:-1].split("] [")
            # (printed with 17 significant digits: the doubles themselves)
            assert np.array_equal(_list(xi).reshape(k, k), want["xi"][b, :k, :k]), (extra, b)
            assert np.array_equal(_list(occ), want["occ"][b, :k]) and np.array_equal(_list(occ_y), want["occ_y"][b, :k]), (extra, b)
            assert np.array_equal(_list(occ_yy), want["occ_yy"][b, :k]), (extra, b)
    # no stream; neither history nor masses: refused by name
    q = subprocess.run(base + ["--running_stats"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--running_stats" in q.stderr and "--stream_chunk" in q.stderr
    q = subprocess.run(base + ["--running_stats", "--stream_chunk", "7", "--filtering_only"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--running_stats" in q.stderr and "--keep_masses" in q.stderr
