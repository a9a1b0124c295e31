"""Decoding through cpprob_main --batch_tables_file ... --decode [--decode_lag L] (Options::map_decode, ::decode_lag;
cpprob::gpu::hmm_table_batch, HmmTableStream, hmm_table_fit): the rows printed after the statistics are the C ABI's, one shot and fed
--stream_chunk K observes at a time, and what the C ABI refuses is refused with a message."""
import json
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
LAG = 2


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def _run(args, ok=True):
    p = subprocess.run([MAIN] + args, capture_output=True, text=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout if ok else p.stderr


def _rows(out, plain, name):
    lines = out.strip().splitlines()
    assert lines[:2] == plain.strip().splitlines()[:2], "%s: --decode changed the statistics" % name
    rows = [ln.split() for ln in lines[2:4]]
    assert [r[:2] for r in rows] == [["decode", "0"], ["decode", "1"]], out
    # (printed with 17 significant digits: the doubles themselves)
    return [np.array([int(v) for v in r[3:]], np.int32) for r in rows], np.array([float(r[2]) for r in rows])


def test_cli_prints_the_python_calls_rows(engine, tmp_path):
    n, seed = 700, 12
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [11, 4]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    base = ["--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt"]
    plain = {"once": _run(base), "kept": _run(base + ["--filtering_only", "--keep_masses"])}
    plain["stream"] = plain["once"]                                # (--stream_chunk: the same output)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_run(np.arange(seed, seed + 2, dtype=np.uint64))
    paths, score = engine.batch_decode()
    st, _ = engine.batch_decode_lag(LAG)
    for name, extra in (("once", []), ("stream", ["--stream_chunk", "2"]), ("kept", ["--filtering_only", "--keep_masses"])):
        got, sc = _rows(_run(base + ["--decode"] + extra), plain[name], name)
        assert all(np.array_equal(x, y) for x, y in zip(got, paths)) and np.array_equal(sc, score), name
        if name != "kept":
            got, sc = _rows(_run(base + ["--decode", "--decode_lag", str(LAG)] + extra), plain[name], name)
            assert all(np.array_equal(got[b], st[b, :T]) for b, T in enumerate(Ts)) and np.array_equal(sc, score), name + ", lag"
    objs = [json.loads(ln) for ln in _run(base + ["--decode", "--json"]).strip().splitlines()]
    assert [o["map_path"] for o in objs] == [p.tolist() for p in paths] and [o["map_score"] for o in objs] == score.tolist()
    # with --em_iterations the decode is that of the fitted tables, run with the keys seed + iterations
    out = _run(base + ["--decode", "--em_iterations", "2"]).strip().splitlines()
    assert len(out) == 6
    fit_m = np.array([[float(v) for v in ln.split("] [")[0].strip("[]").split()] for ln in out[4:]])
    fit_t = np.array([[float(v) for v in ln.split("] [")[1].strip("[]").split()] for ln in out[4:]]).reshape(2, 3, 3)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(fit_m, fit_t))
    engine.batch_run(np.arange(seed + 2, seed + 4, dtype=np.uint64))
    fp, fs = engine.batch_decode()
    rows = [ln.split() for ln in out[2:4]]
    assert all([int(v) for v in rows[b][3:]] == fp[b].tolist() and float(rows[b][2]) == fs[b] for b in range(2))
    # what the C ABI refuses is refused with a message
    assert "--keep_masses" in _run(base + ["--decode", "--filtering_only"], ok=False)
    assert "--decode_lag delays a decode" in _run(base + ["--decode_lag", "1"], ok=False)
    assert "--decode serves the batch modes" in _run(["--smc", "--model", "hmm16", "--observes", "1", "--decode"], ok=False)
