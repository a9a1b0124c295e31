"""Trajectory statistics through cpprob_main --batch_tables_file ... --trajectory_stats M [--draw_index D]
(cpprob::gpu::Options::trajectory_stats): the M lines a problem it prints after the usual output are Engine.batch_traj_stats' doubles,
with the history, fed in pieces (--stream_chunk) and, --filtering_only --keep_masses, from the masses alone; without either the flag
is refused by name.  --batch_observes_file (cpprob::gpu::inference_batch, the three-state HMM) prints the same lines."""
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


def test_cli_prints_the_engines_records(engine, tmp_path):
    n, seed, M, D, k = 300, 12, 3, 5, 3
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [40, 17]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    base = [MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt"]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_run(np.arange(seed, seed + 2, dtype=np.uint64))
    want = engine.batch_traj_stats(M, D, obs)
    ev = [s["log_evidence"] for s in engine.batch_results()[0]]
    for extra in ([], ["--filtering_only", "--keep_masses"], ["--stream_chunk", "7"]):      # (the last: cpprob::gpu::HmmTableStream)
        p = subprocess.run(base + ["--trajectory_stats", str(M), "--draw_index", str(D)] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 2 + 2 * M, p.stdout
        for b in range(2):
            assert _list(lines[b])[0] == ev[b], (extra, b)
            for j in range(M):
                line = lines[2 + b * M + j]
                assert line.startswith("[") and line.endswith("]"), line
                xi, occ, occ_y, occ_yy = line[1:-1].split("] [")
                # (printed with 17 significant digits: the doubles themselves)
                assert np.array_equal(_list(xi).reshape(k, k), want["xi"][b, j, :k, :k]), (extra, b, j)
                assert np.array_equal(_list(occ), want["occ"][b, j, :k]) and np.array_equal(_list(occ_y), want["occ_y"][b, j, :k]), (extra, b, j)
                assert np.array_equal(_list(occ_yy), want["occ_yy"][b, j, :k]), (extra, b, j)
    assert want["occ"].sum(axis=2).tolist() == [[40.0] * M, [17.0] * M]
    # neither history nor masses: refused by name
    q = subprocess.run(base + ["--trajectory_stats", str(M), "--filtering_only"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--trajectory_stats" in q.stderr and "--keep_masses" in q.stderr


def test_cli_prints_the_records_of_an_observes_batch(engine, tmp_path):
    """One hmm<16> problem a line through cpprob::gpu::inference_batch: M lines a problem over the model's three states."""
    from oracle import exact
    B, T, n, seed, M = 3, 16, 500, 40, 2
    obs = np.array([exact.simulate_hmm(T, 700 + b) for b in range(B)])
    (tmp_path / "batch.txt").write_text("".join(_numbers(row) + "\n" for row in obs))
    p = subprocess.run([MAIN, "--model_folder", str(tmp_path), "--model", "hmm16", "--smc", "--n_samples", str(n), "--seed", str(seed), "--ess_threshold", "2.0",
                        "--batch_observes_file", "batch.txt", "--trajectory_stats", str(M)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("[")]
    assert len(lines) == B * M, p.stdout
    engine.batch_begin(cp.MODEL_HMM3, obs, n)
    engine.batch_run(np.arange(seed, seed + B, dtype=np.uint64))
    want = engine.batch_traj_stats(M, 0, obs)
    for b in range(B):
        for j in range(M):
            xi, occ, occ_y, occ_yy = lines[b * M + j][1:-1].split("] [")
            assert np.array_equal(_list(xi).reshape(3, 3), want["xi"][b, j, :3, :3]) and np.array_equal(_list(occ), want["occ"][b, j, :3]), (b, j)
            assert np.array_equal(_list(occ_y), want["occ_y"][b, j, :3]) and np.array_equal(_list(occ_yy), want["occ_yy"][b, j, :3]), (b, j)
