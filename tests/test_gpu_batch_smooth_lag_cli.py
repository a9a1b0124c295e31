"""Fixed-lag smoothing through cpprob_main --batch_tables_file ... --smoothing_lag L (Options::smoothing_lag;
cpprob::gpu::hmm_table_batch, HmmTableStream): fed --stream_chunk K observes at a time the stream asks for the steps not yet final
only and prints, byte for byte, what the one-shot batch prints -- the C ABI's fixed-lag marginals."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def _run(args):
    p = subprocess.run([MAIN] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_cli_stream_prints_the_one_shot_batchs_fixed_lag_rows(engine, tmp_path):
    n, seed, lag = 700, 12, 2
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [11, 4]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    text = "".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2))
    out = {}
    for name, extra in (("once", ["--smoothing_lag", str(lag)]), ("stream", ["--smoothing_lag", str(lag), "--stream_chunk", "3"]), ("plain", [])):
        d = tmp_path / name
        d.mkdir()
        (d / "tables.txt").write_text(text)
        out[name] = _run(["--model_folder", str(d), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt"] + extra)
    assert out["stream"] == out["once"], "the chunked stream prints other numbers than the one-shot batch"
    assert out["once"] != out["plain"], "--smoothing_lag changed nothing"
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_run(np.arange(seed, seed + 2, dtype=np.uint64))
    summ = engine.batch_results()[0]
    marg, _ = engine.batch_smooth_lag(lag)
    lines = out["once"].strip().splitlines()
    assert len(lines) == 2, out["once"]
    for b in range(2):
        got = np.array([float(v) for v in lines[b].split()])
        assert got[0] == summ[b]["log_evidence"], b
        # (printed with 17 significant digits: the doubles themselves)
        assert np.array_equal(got[1:].reshape(Ts[b], 3), marg[b, :Ts[b], :3]), b
