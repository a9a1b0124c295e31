"""cpprob_main --batch_tables_file ... --filtering_only --keep_masses (Options::keep_masses): the batch modes smooth and fit
filtering-only batches from the masses the runs keep, and print what the same command prints with the particle store kept; without
--keep_masses the filtering-only forms are refused as before."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_masses_cli")
    means = np.array([[-2.0, 0.0, 2.5], [-1.0, 0.5, 3.0]])
    trans = np.array([[[0.8, 0.1, 0.1], [0.2, 0.6, 0.2], [0.1, 0.3, 0.6]], [[0.5, 0.5, 0.0], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]]])
    rng = np.random.default_rng(4)
    obs = [means[b][rng.integers(0, 3, T)] + rng.standard_normal(T) for b, T in enumerate([23, 9])]
    (d / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(2)))
    return str(d)


def _run(folder, *flags):
    return subprocess.run([MAIN, "--model_folder", folder, "--smc", "--ess_threshold", "2", "--n_samples", "300", "--seed", "12", "--batch_tables_file", "tables.txt"] + list(flags),
                          capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("flags,lines", [(["--backward_smoothing"], 2), (["--smoothing_lag", "2"], 2), (["--backward_smoothing", "--em_iterations", "2"], 4),
                                         (["--smoothing_lag", "2", "--stream_chunk", "4"], 2)])
def test_filtering_only_with_masses_prints_what_the_kept_history_prints(folder, flags, lines):
    kept = _run(folder, *flags)
    assert kept.returncode == 0, kept.stdout[-2000:] + kept.stderr[-2000:]
    masses = _run(folder, "--filtering_only", "--keep_masses", *flags)
    assert masses.returncode == 0, masses.stdout[-2000:] + masses.stderr[-2000:]
    assert len(kept.stdout.strip().splitlines()) == lines, kept.stdout
    assert masses.stdout == kept.stdout
    # without --keep_masses the filtering-only form fails as before
    plain = _run(folder, "--filtering_only", *flags)
    assert plain.returncode != 0 and "filtering-only run" in plain.stderr and plain.stdout.strip() == "", plain.stderr[-2000:]


def test_the_printed_predicts_are_the_smoothers_not_the_filters(folder):
    smoothed = _run(folder, "--filtering_only", "--keep_masses", "--backward_smoothing")
    filtered = _run(folder, "--filtering_only", "--keep_masses")
    assert smoothed.returncode == 0 and filtered.returncode == 0
    assert smoothed.stdout != filtered.stdout and len(filtered.stdout.strip().splitlines()) == 2
    assert filtered.stdout == _run(folder, "--filtering_only").stdout         # (the bit alone changes nothing a run prints)


@pytest.mark.parametrize("extra", [[], ["--stream_chunk", "4"]])
def test_backward_trajectories_are_dumped_from_the_masses(folder, tmp_path, extra):
    """--batch_dump --backward_trajectories M: the files hold backward-simulated trajectories, which need the masses alone -- the same
    bytes with and without the particle store.  The lineage dump of a filtering-only batch stays refused."""
    import shutil
    got = {}
    for name, flags in (("kept", []), ("masses", ["--filtering_only", "--keep_masses"])):
        d = tmp_path / name
        d.mkdir()
        shutil.copy(os.path.join(folder, "tables.txt"), str(d / "tables.txt"))
        p = _run(str(d), "--backward_smoothing", "--backward_trajectories", "6", "--batch_dump", *(flags + extra))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        got[name] = [p.stdout] + [open(str(d / ("post_smc_%d.%s" % (b, ext))), "rb").read() for b in range(2) for ext in ("int", "ids")]
    assert got["masses"] == got["kept"] and all(len(x) > 0 for x in got["kept"])
    d = tmp_path / "lineages"
    d.mkdir()
    shutil.copy(os.path.join(folder, "tables.txt"), str(d / "tables.txt"))
    p = _run(str(d), "--filtering_only", "--keep_masses", "--batch_dump", *extra)
    assert p.returncode != 0 and "keeps no traces to dump" in p.stderr and not os.path.exists(str(d / "post_smc_0.int")), p.stderr[-2000:]
