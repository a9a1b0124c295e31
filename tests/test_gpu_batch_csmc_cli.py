"""cpprob_main --batch_tables_file ... --filtering_only --keep_masses --conditional_paths FILE (Options::conditional_paths): the
run of the batch is the conditional SMC run on the paths of FILE, and --trajectory_stats prints the records the Python route
computes on the same inputs; without --keep_masses hmm_table_batch refuses."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
SEED, N, K = 12, 300, 3


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_csmc_cli")
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    obs = [means[b][rng.integers(0, K, T)] + rng.standard_normal(T) for b, T in enumerate([23, 9])]
    paths = [rng.integers(0, K, len(o)).astype(np.int32) for o in obs]
    (d / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    (d / "paths.txt").write_text("".join(" ".join(str(int(s)) for s in p) + "\n" for p in paths))
    return str(d), means, trans, obs, paths


def _run(folder, *flags):
    return subprocess.run([MAIN, "--model_folder", folder, "--smc", "--ess_threshold", "2", "--n_samples", str(N), "--seed", str(SEED), "--batch_tables_file", "tables.txt"] + list(flags),
                          capture_output=True, text=True, timeout=600)


def _records(lines):
    """[[xi k x k], [occ], [occ_y], [occ_yy]] of every printed line, as floats."""
    return [[[float(v) for v in part.strip("[] ").split()] for part in line.split("] [")] for line in lines]


def test_trajectory_stats_of_a_conditional_run_are_the_python_routes(engine, case):
    folder, means, trans, obs, paths = case
    p = _run(folder, "--filtering_only", "--keep_masses", "--conditional_paths", "paths.txt", "--trajectory_stats", "2", "--draw_index", "3")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 2 + 4, p.stdout
    assert [float(line.split()[0]) for line in lines[:2]] == [0.0, 0.0] and all(len(line.split()) == 1 for line in lines[:2]), "a conditional run keeps no books"
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=(means, trans), keep_history=False, keep_masses=True)
    engine.batch_run_conditional(np.array([SEED, SEED + 1], np.uint64), paths)
    st = engine.batch_traj_stats(2, draw_index=3, observes=obs)
    got = _records(lines[2:])
    for b in range(2):
        for j in range(2):
            rec = got[2 * b + j]
            assert rec[0] == st["xi"][b, j, :K, :K].reshape(-1).tolist() and rec[1] == st["occ"][b, j, :K].tolist()
            assert rec[2] == st["occ_y"][b, j, :K].tolist() and rec[3] == st["occ_yy"][b, j, :K].tolist()
    # another path, another run
    other = _run(folder, "--filtering_only", "--keep_masses", "--trajectory_stats", "2", "--draw_index", "3")
    assert other.returncode == 0 and other.stdout.strip().splitlines()[2:] != lines[2:]


def test_smoothing_of_a_conditional_run_prints_the_python_routes_marginals(engine, case):
    folder, means, trans, obs, paths = case
    p = _run(folder, "--filtering_only", "--keep_masses", "--conditional_paths", "paths.txt", "--backward_smoothing")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=(means, trans), keep_history=False, keep_masses=True)
    engine.batch_run_conditional(np.array([SEED, SEED + 1], np.uint64), paths)
    marg, _ = engine.batch_smooth()
    for b, line in enumerate(p.stdout.strip().splitlines()):
        vals = [float(v) for v in line.split()]
        assert vals[0] == 0.0 and vals[1:] == marg[b, :len(obs[b]), :K].reshape(-1).tolist()


def test_refused_without_keep_masses(case):
    p = _run(case[0], "--filtering_only", "--conditional_paths", "paths.txt")
    assert p.returncode != 0 and "conditional_paths" in p.stderr and "keep_masses" in p.stderr and p.stdout.strip() == ""
