"""Tied tables through cpprob_main --batch_tables_file ... --em_iterations N --tie_groups "[0 1 0 1]" (cpprob::gpu::Options::tie_groups):
the fitted tables printed are the ones cpprob_amd.hmm_table_em(groups=...) returns on its host route for the same input, to the 17
significant digits printed -- that route pools in numpy, the CLI through the device's kernel, so the two check each other --, with and
without --em_on_device and with --emission_scales --learn_scales; --tie_tables is --tie_groups of all zeros; unequal input tables of a
group are refused by name."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
GROUPS = [0, 1, 0, 1]
TS = [40, 17, 9, 33]


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def _list(text):
    return np.array([float(v) for v in text.split()])


def _fitted(line):
    assert line.startswith("[") and line.endswith("]"), line
    return [_list(part) for part in line[1:-1].split("] [")]


def _case():
    g_means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    g_sigmas = np.array([[0.5, 1.0, 1.5], [1.2, 0.7, 2.0]])
    g_trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    means, sigmas, trans = g_means[GROUPS], g_sigmas[GROUPS], g_trans[GROUPS]
    rng = np.random.default_rng(4)
    obs = []
    for b, T in enumerate(TS):
        x = rng.integers(0, 3, T)
        obs.append(means[b][x] + sigmas[b][x] * rng.standard_normal(T))
    return means, sigmas, trans, obs


def test_cli_prints_the_tables_of_the_python_host_route(engine, tmp_path):
    n, seed, iters = 300, 12, 4
    means, sigmas, trans, obs = _case()
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(4)))
    (tmp_path / "scaled.txt").write_text("".join("%s %s %s %s\n" % (_numbers(means[b]), _numbers(sigmas[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(4)))
    seeds = np.arange(seed, seed + 4, dtype=np.uint64)

    def run(file, extra, ok=True):
        p = subprocess.run([MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(n), "--seed", str(seed), "--batch_tables_file", file,
                            "--em_iterations", str(iters)] + extra, capture_output=True, text=True, timeout=600)
        assert (p.returncode == 0) == ok, p.stdout[-2000:] + p.stderr[-2000:]
        return p.stdout.strip().splitlines() if ok else p.stderr

    tie = ["--tie_groups", "[0 1 0 1]"]
    m, t, ev = cp.hmm_table_em(engine, obs, means, trans, n, seeds, iters, groups=GROUPS)
    outputs = []
    for extra in (tie, tie + ["--em_on_device"]):
        lines = run("tables.txt", extra)
        assert len(lines) == 8, lines
        for b in range(4):
            assert _list(lines[b])[0] == ev[-1, b], (extra, b)
            got = _fitted(lines[4 + b])
            assert len(got) == 2 and np.array_equal(got[0], m[-1, b]) and np.array_equal(got[1].reshape(3, 3), t[-1, b]), (extra, b)
        assert lines[4] == lines[6] and lines[5] == lines[7] and lines[4] != lines[5]          # a group's members print one table
        outputs.append(lines)
    assert outputs[0] == outputs[1]
    # untied, the same problems end elsewhere
    assert run("tables.txt", [])[4:] != outputs[0][4:]
    # emission scales, fitted too
    m, t, ev, sg = cp.hmm_table_em(engine, obs, means, trans, n, seeds, iters, sigmas0=sigmas, groups=GROUPS)
    for extra in (tie, tie + ["--em_on_device"]):
        lines = run("scaled.txt", ["--emission_scales", "--learn_scales"] + extra)
        assert len(lines) == 8, lines
        for b in range(4):
            assert _list(lines[b])[0] == ev[-1, b], (extra, b)
            got = _fitted(lines[4 + b])
            assert len(got) == 3 and np.array_equal(got[0], m[-1, b]) and np.array_equal(got[1].reshape(3, 3), t[-1, b]) and np.array_equal(got[2], sg[-1, b]), (extra, b)
    assert not np.array_equal(sg[-1], sigmas)
    # --tie_tables is --tie_groups of all zeros (the four input tables made equal)
    (tmp_path / "one.txt").write_text("".join("%s %s %s\n" % (_numbers(means[0]), _numbers(trans[0]), _numbers(obs[b])) for b in range(4)))
    all_tied = run("one.txt", ["--tie_tables"])
    assert all_tied == run("one.txt", ["--tie_groups", "[0 0 0 0]"]) and len(set(all_tied[4:])) == 1
    m, t, ev = cp.hmm_table_em(engine, obs, np.tile(means[0], (4, 1)), np.tile(trans[0], (4, 1, 1)), n, seeds, iters, groups=[0, 0, 0, 0])
    assert np.array_equal(_fitted(all_tied[4])[0], m[-1, 0]) and np.array_equal(_fitted(all_tied[7])[1].reshape(3, 3), t[-1, 3])
    # refusals, by name: unequal tables in a group, a list of the wrong length, an unused id
    err = run("tables.txt", ["--tie_tables"], ok=False)
    assert "group 0" in err
    err = run("tables.txt", ["--tie_groups", "[0 1 0]"], ok=False)
    assert "--tie_groups" in err
    err = run("tables.txt", ["--tie_groups", "[0 2 0 2]"], ok=False)
    assert "unused" in err
