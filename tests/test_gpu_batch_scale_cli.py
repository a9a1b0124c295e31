"""Emission scales through cpprob_main --batch_tables_file ... --emission_scales (cpprob::gpu::HmmTable::sigmas, Options::learn_scales,
Options::scale_floor): every line of the tables file carries [means] [sigmas] [transition] [observes]; with --em_iterations N
--learn_scales and with --stream_chunk K --online_em --learn_scales the fitted sigmas are printed behind the fitted tables and are the
ones cpprob_amd.hmm_table_em and cpprob_amd.hmm_table_online_em return for the same input, to the 17 significant digits printed;
without --learn_scales the sigmas stay; the flags are refused by name where they have nothing to act on."""
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
    m, t, s = line[1:-1].split("] [")
    return _list(m), _list(t).reshape(k, k), _list(s)


def test_cli_prints_the_sigmas_the_python_routes_return(engine, tmp_path):
    n, seed, k, chunk = 300, 12, 3, 4
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    sigmas = np.array([[0.5, 1.0, 1.5], [1.2, 0.7, 2.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    Ts = [40, 17]
    obs = []
    for b, T in enumerate(Ts):
        x = rng.integers(0, 3, T)
        obs.append(means[b][x] + sigmas[b][x] * rng.standard_normal(T))
    (tmp_path / "tables.txt").write_text("".join("%s %s %s %s\n" % (_numbers(means[b]), _numbers(sigmas[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    base = [MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", "tables.txt",
            "--emission_scales"]
    seeds = np.arange(seed, seed + 2, dtype=np.uint64)

    def run(extra):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 4, p.stdout
        return lines
    # particle EM: --em_iterations 2 --learn_scales, host loop and --em_on_device; another floor; the sigmas kept without the flag
    for extra, floor in ((["--learn_scales"], 1e-3), (["--learn_scales", "--em_on_device"], 1e-3), (["--learn_scales", "--scale_floor", "1.25"], 1.25)):
        m, t, ev, sg = cp.hmm_table_em(engine, obs, means, trans, n, seeds, 2, sigmas0=sigmas, sigma_floor=floor)
        lines = run(["--em_iterations", "2"] + extra)
        for b in range(2):
            assert _list(lines[b])[0] == ev[-1, b], (extra, b)
            got = _fitted(lines[2 + b], k)
            assert np.array_equal(got[0], m[-1, b]) and np.array_equal(got[1], t[-1, b]) and np.array_equal(got[2], sg[-1, b]), (extra, b)
        assert not np.array_equal(sg[-1], sigmas) and (floor < 1.0 or np.any(sg[-1] == 1.25))
    lines = run(["--em_iterations", "2"])
    assert all(np.array_equal(_fitted(lines[2 + b], k)[2], sigmas[b]) for b in range(2))
    # online EM: --stream_chunk 4 --online_em --learn_scales, with the history and from the masses alone
    for extra, kw in ((["--em_burn_in", "8"], dict(t_min=8, keep_history=True)),
                      (["--em_burn_in", "8", "--filtering_only", "--keep_masses", "--scale_floor", "0.01"], dict(t_min=8, keep_history=False, sigma_floor=0.01))):
        m, t, st, sums, sg = cp.hmm_table_online_em(engine, obs, (means, trans, sigmas), n, seeds, chunk, **kw)
        assert not st.any() and not np.array_equal(sg[-1], sigmas)
        lines = run(["--stream_chunk", str(chunk), "--online_em", "--learn_scales"] + extra)
        for b in range(2):
            assert _list(lines[b])[0] == sums[b]["log_evidence"], (extra, b)
            got = _fitted(lines[2 + b], k)
            assert np.array_equal(got[0], m[-1, b]) and np.array_equal(got[1], t[-1, b]) and np.array_equal(got[2], sg[-1, b]), (extra, b)
    lines = run(["--stream_chunk", str(chunk), "--online_em", "--em_burn_in", "8"])      # (a plain arming: means and rows move, the sigmas stay)
    assert all(np.array_equal(_fitted(lines[2 + b], k)[2], sigmas[b]) and not np.array_equal(_fitted(lines[2 + b], k)[0], means[b]) for b in range(2))
    # the plain batch of scaled tables: the evidence of the Python route
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans, sigmas))
    engine.batch_run(seeds)
    p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and [_list(x)[0] for x in p.stdout.strip().splitlines()] == [s["log_evidence"] for s in engine.batch_results()[0]]
    # refusals, by name
    q = subprocess.run(base + ["--learn_scales"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--learn_scales" in q.stderr and "--em_iterations" in q.stderr
    q = subprocess.run([a for a in base if a != "--emission_scales"] + ["--em_iterations", "2", "--learn_scales"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "--learn_scales" in q.stderr and "--emission_scales" in q.stderr
    (tmp_path / "three.txt").write_text("%s %s %s\n" % (_numbers(means[0]), _numbers(trans[0]), _numbers(obs[0])))
    q = subprocess.run(base[:-3] + ["--batch_tables_file", "three.txt", "--emission_scales"], capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "[sigmas]" in q.stderr
