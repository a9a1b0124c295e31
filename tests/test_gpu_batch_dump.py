"""Posterior files of a batch through cpprob_main --batch_dump (cpprob::gpu::inference_batch, hmm_table_batch, HmmTableStream::dump):
problem b's <generated_file>_smc_<b>.int / .ids are, byte for byte, the files a single run of that problem writes, and the text
the reference grammar gives for Engine.batch_paths of the same problems."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp
from oracle import exact

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def _run(args):
    p = subprocess.run([MAIN] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p


def _read(folder, name):
    with open(os.path.join(str(folder), name), "rb") as f:
        return f.read()


def test_batch_observes_dump_is_the_single_runs_files(tmp_path):
    B, T, n, seed = 3, 16, 600, 40
    obs = [exact.simulate_hmm(T, 800 + b) for b in range(B)]
    batch = tmp_path / "batch"
    batch.mkdir()
    (batch / "batch.txt").write_text("".join(_numbers(o) + "\n" for o in obs))
    common = ["--model", "hmm16", "--smc", "--ess_threshold", "2", "--n_samples", str(n)]
    _run(["--model_folder", str(batch)] + common + ["--seed", str(seed), "--batch_observes_file", "batch.txt", "--batch_dump"])
    for b in range(B):
        single = tmp_path / ("single%d" % b)               # (a fresh directory a run: the dump appends)
        single.mkdir()
        _run(["--model_folder", str(single)] + common + ["--seed", str(seed + b), "--observes", _numbers(obs[b])])
        want_int, want_ids = _read(single, "post_smc.int"), _read(single, "post_smc.ids")
        assert want_int.count(b"\n") == n and want_ids.count(b"\n") > 0
        assert _read(batch, "post_smc_%d.int" % b) == want_int, b
        assert _read(batch, "post_smc_%d.ids" % b) == want_ids, b
    # without --batch_dump no file appears
    quiet = tmp_path / "quiet"
    quiet.mkdir()
    (quiet / "batch.txt").write_text("".join(_numbers(o) + "\n" for o in obs))
    _run(["--model_folder", str(quiet)] + common + ["--seed", str(seed), "--batch_observes_file", "batch.txt"])
    assert sorted(os.listdir(str(quiet))) == ["batch.txt"]


def _render(paths, logw):
    """dump_posterior's grammar for int predicts with ids 0 .. T-1: ([(id v) ...] logw), scientific with 15 digits."""
    T, m = paths.shape
    return "".join("([" + " ".join("(%d %d)" % (t, paths[t, i]) for t in range(T)) + "] %.15e)\n" % logw[i] for i in range(m)).encode()


def test_batch_tables_dump_at_once_streamed_and_capped(engine, tmp_path):
    n, seed = 700, 12
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [5, 3]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    text = "".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2))
    folders = {}
    for name, extra in (("once", []), ("stream", ["--stream_chunk", "2"]), ("capped", ["--dump_max_particles", "7"])):
        d = tmp_path / name
        d.mkdir()
        (d / "tables.txt").write_text(text)
        _run(["--model_folder", str(d), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt", "--batch_dump"] + extra)
        folders[name] = d
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_run(np.arange(seed, seed + 2, dtype=np.uint64))
    paths, logw = engine.batch_paths()
    for b in range(2):
        want_int = _render(paths[b], logw[b])
        want_ids = "".join("state[%d]\n" % t for t in range(Ts[b])).encode()
        for name in ("once", "stream"):
            assert _read(folders[name], "post_smc_%d.int" % b) == want_int, (name, b)
            assert _read(folders[name], "post_smc_%d.ids" % b) == want_ids, (name, b)
        # Options::dump_max_particles = 7: the first seven traces
        capped = _read(folders["capped"], "post_smc_%d.int" % b)
        assert capped.count(b"\n") == 7 and capped == b"".join(want_int.splitlines(True)[:7]), b
        assert _read(folders["capped"], "post_smc_%d.ids" % b) == want_ids
