"""Forecasts through cpprob_main --batch_tables_file ... --forecast H --forecast_trajectories M (Options::forecast_horizon,
::forecast_trajectories; cpprob::gpu::hmm_table_batch, HmmTableStream): the rows printed after the statistics are the C ABI's, one
shot and fed --stream_chunk K observes at a time."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
H, M = 3, 5


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def _run(args, ok=True):
    p = subprocess.run([MAIN] + args, capture_output=True, text=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout if ok else p.stderr


def test_cli_prints_the_python_calls_rows(engine, tmp_path):
    n, seed = 700, 12
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [11, 4]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    base = ["--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt"]
    fc = ["--forecast", str(H), "--forecast_trajectories", str(M)]
    out = {"once": _run(base + fc), "stream": _run(base + fc + ["--stream_chunk", "2"]), "plain": _run(base)}
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_run(np.arange(seed, seed + 2, dtype=np.uint64))
    marg, traj = engine.batch_forecast(H, M)
    for name in ("once", "stream"):
        lines = out[name].strip().splitlines()
        assert lines[:2] == out["plain"].strip().splitlines(), "%s: --forecast changed the statistics" % name
        assert len(lines) == 2 + 2 * (H + M), out[name]
        rows = [ln.split() for ln in lines[2:]]
        for b in range(2):
            mine = rows[b * (H + M):(b + 1) * (H + M)]
            for h in range(H):
                assert mine[h][:3] == ["forecast", str(b), str(h + 1)], mine[h]
                # (printed with 17 significant digits: the doubles themselves)
                assert np.array_equal(np.array([float(v) for v in mine[h][3:]]), marg[b, h, :3]), (name, b, h)
            for j in range(M):
                assert mine[H + j][:3] == ["future", str(b), str(j)], mine[H + j]
                assert [int(v) for v in mine[H + j][3:]] == traj[b, :, j].tolist(), (name, b, j)
    # what the C ABI refuses is refused with a message
    err = _run(base + ["--forecast", str(H), "--filtering_only"], ok=False)
    assert "keep_masses" in err
    err = _run(base + ["--forecast_trajectories", "4"], ok=False)
    assert "forecast_horizon" in err
    kept = _run(base + fc + ["--filtering_only", "--keep_masses"])
    assert kept.strip().splitlines()[2:] == out["once"].strip().splitlines()[2:], "a keep_masses batch prints other forecast rows"
