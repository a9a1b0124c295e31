"""Backward smoothing through cpprob_main --batch_tables_file ... --backward_smoothing --backward_trajectories M --batch_dump
(Options::backward_smoothing, ::backward_trajectories; cpprob::gpu::hmm_table_batch, HmmTableStream): the printed statistics are the
C ABI's marginals and the dumped traces its trajectories, with equal weights."""
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
    return p


def _read(folder, name):
    with open(os.path.join(str(folder), name), "rb") as f:
        return f.read()


def _render(traj):
    """dump_posterior's grammar for int predicts with ids 0 .. T-1 and log-weight 0: ([(id v) ...] 0.0e+00)."""
    T, m = traj.shape
    return "".join("([" + " ".join("(%d %d)" % (t, traj[t, i]) for t in range(T)) + "] %.15e)\n" % 0.0 for i in range(m)).encode()


def test_cli_statistics_and_traces_are_the_c_abis(engine, tmp_path):
    n, seed, M = 700, 12, 8
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [5, 3]
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    text = "".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2))
    out, folders = {}, {}
    for name, extra in (("once", []), ("stream", ["--stream_chunk", "2"])):
        d = tmp_path / name
        d.mkdir()
        (d / "tables.txt").write_text(text)
        out[name] = _run(["--model_folder", str(d), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt",
                          "--backward_smoothing", "--backward_trajectories", str(M), "--batch_dump"] + extra).stdout
        folders[name] = d
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_run(np.arange(seed, seed + 2, dtype=np.uint64))
    summ, stats, _, _ = engine.batch_results()
    marg, traj = engine.batch_smooth(M)
    assert not np.array_equal(marg, stats), "the backward marginals should differ from the lineage statistics"
    for name in ("once", "stream"):
        lines = out[name].strip().splitlines()
        assert len(lines) == 2, out[name]
        for b in range(2):
            got = np.array([float(v) for v in lines[b].split()])
            assert got[0] == summ[b]["log_evidence"], (name, b)
            # (printed with 17 significant digits: the doubles themselves)
            assert np.array_equal(got[1:].reshape(Ts[b], 3), marg[b, :Ts[b], :3]), (name, b)
            assert _read(folders[name], "post_smc_%d.int" % b) == _render(traj[b]), (name, b)
            assert _read(folders[name], "post_smc_%d.ids" % b) == "".join("state[%d]\n" % t for t in range(Ts[b])).encode(), (name, b)
    # without the flags the output is the lineage walk's, as before
    d = tmp_path / "plain"
    d.mkdir()
    (d / "tables.txt").write_text(text)
    plain = _run(["--model_folder", str(d), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt"]).stdout
    for b, line in enumerate(plain.strip().splitlines()):
        got = np.array([float(v) for v in line.split()])
        assert np.array_equal(got[1:].reshape(Ts[b], 3), stats[b, :Ts[b], :3]), b
