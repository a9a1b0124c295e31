"""csrc/batch_pass_plan.hpp -- what batch_smooth_enqueue decides on the host for one batch pass -- as host code: the header is built
with tests/host_kernels/batch_pass_plan_main.cpp as a stand-alone program (g++ -std=c++17 -O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=undefined), run as a child process over a file of cases, and every descriptor field, grid, byte count and the
early return must equal tests/pass_plan_ref.py's.  Nothing is loaded into python and nothing runs on a GPU.

The case file: the number of cases; a case is {kind, B, online, kept, T_max, spp, lag, 1: from is given, n_rows, horizon, n_traj,
1: the doubles output is there, 1: the entries output is there} and B rows {T, n, store, capacity, counted, decoded, ostats_done,
from}.  The output a case: "case i", "head" and Head's fields and, unless the call is done, "tail" and Tail's and a "desc" line a
problem."""
import os
import re
import subprocess

import pytest

import pass_plan_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")

LENS, NS = [23, 9, 1], [70, 1, 300]
OUTPUTS = [(True, True), (True, False), (False, True)]               # (the doubles, the entries): both, the former only, the latter only


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_pass_plan_host"))
    exe = os.path.join(d, "batch_pass_plan_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-I", CSRC,
           os.path.join(HERE, "batch_pass_plan_main.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr.strip() == "", p.stderr[-4000:]

    def run(cases):
        """[(Head, Tail or None, [Desc] or None)] of the cases [(Batch, kind, keyword arguments of pass_plan_ref.plan)]."""
        lines = [str(len(cases))]
        for bt, kind, kw in cases:
            frm = kw.get("frm")
            lines.append(" ".join(str(int(x)) for x in (P.KINDS.index(kind), bt.B, bt.online, bt.kept, bt.T_max, bt.spp, kw.get("lag", 0), frm is not None,
                                                        kw.get("n_rows", 0), kw.get("horizon", 0), kw.get("n_traj", 0), kw.get("doubles", True), kw.get("entries", True))))
            for b in range(bt.B):
                lines.append("%d %d %d %d %d %d %d %d" % (bt.lens[b], bt.ns[b], bt.store[b], bt.caps[b], bt.counted[b], bt.decoded[b], bt.ostats_done[b],
                                                          frm[b] if frm is not None else 0))
        fin = os.path.join(d, "cases.txt")
        open(fin, "w").write("\n".join(lines) + "\n")
        p = subprocess.run([exe, fin], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        got, rows = [], [l.split() for l in p.stdout.splitlines()]
        for r in rows:
            vals = [int(x) for x in r[1:]]
            if r[0] == "case":
                assert vals == [len(got)]
                got.append([None, None, None])
            elif r[0] == "head":
                got[-1][0] = P.Head(*vals)
            elif r[0] == "tail":
                got[-1][1], got[-1][2] = P.Tail(*vals), []
            else:
                assert r[0] == "desc"
                got[-1][2].append(P.Desc(*vals))
        assert len(got) == len(cases)
        return [tuple(g) for g in got]
    return run


def check(prog, cases):
    got = prog(cases)
    for (bt, kind, kw), g in zip(cases, got):
        want = P.plan(bt, kind, **kw)
        assert g == want, "%s %s, lengths %s%s%s:\n got  %s\n want %s" % (kind, kw, bt.lens, " online" if bt.online else "", " kept" if bt.kept else "", g, want)
    return got


def every_kind(bt, froms=(None,), lags=(3,), n_traj=5):
    """Every pass over `bt`; the passes that take from / lag at each of them, the passes with two outputs at each combination."""
    cases = [(bt, "stats", {}), (bt, "online_stats", {}), (bt, "traj_stats", dict(n_traj=n_traj))]
    top = max(bt.lens) + 2
    for d, e in OUTPUTS:
        cases += [(bt, "smooth", dict(n_traj=n_traj, doubles=d, entries=e)), (bt, "forecast", dict(horizon=6, n_traj=n_traj, doubles=d, entries=e)),
                  (bt, "decode", dict(doubles=d, entries=e))]
        for frm in froms:
            for lag in lags:
                cases += [(bt, "smooth_lag", dict(lag=lag, frm=frm, n_rows=top, n_traj=n_traj, doubles=d, entries=e)),
                          (bt, "decode_lag", dict(lag=lag, frm=frm, n_rows=top, doubles=d, entries=e))]
    for frm in froms:
        cases.append((bt, "predictive", dict(frm=frm, n_rows=top)))
    assert {k for _, k, _ in cases} == set(P.KINDS)
    return cases


FROMS = (None, [0, 0, 0], [23, 9, 1], [20, 0, 1])
LAGS = (0, 3, 40)


def test_run_batch(prog):
    """from == L, lag + 1 > L; the marginals only, the trajectories only and both, for cfrom."""
    bt = P.Batch(LENS, NS)
    got = check(prog, every_kind(bt, FROMS, LAGS))
    assert all(h.mass_rows == h.word_rows == 33 and not h.done for h, _, _ in got)
    one = check(prog, [(bt, "smooth_lag", dict(lag=3, frm=[20, 0, 1], n_rows=25, n_traj=5, doubles=dd, entries=e)) for dd, e in OUTPUTS])
    assert [[x.cfrom for x in ds] for _, _, ds in one] == [[19, 0, 0], [20, 0, 1], [19, 5, 0]]
    assert [[x.trows for x in one[0][2]], [x.lo for x in one[0][2]]] == [[0, 4, 8], [19, 5, 0]]


def test_online_batch(prog):
    """The tables by capacity, the counting from the watermark; problem 0 has no new step for the running statistics."""
    bt = P.Batch(LENS, NS, caps=[25, 12, 4], counted=[5, 0, 1], decoded=[6, 9, 0], ostats_done=[23, 2, 1])
    got = check(prog, every_kind(bt, FROMS, LAGS))
    assert all(h.mass_rows == h.word_rows == 41 for h, _, _ in got)
    assert all([d.rows for d in ds] == [0, 25, 37] and [d.cfrom for d in ds] == [5, 0, 1] for _, _, ds in got)
    (_, t, ds), = check(prog, [(bt, "online_stats", {})])
    assert t.fresh == 7 and [(d.lo, d.trows) for d in ds] == [(23, 0), (2, 0), (1, 7)] and t.count_gy == 18
    (_, t, ds), = check(prog, [(bt, "decode", {})])
    assert [d.lo for d in ds] == [6, 9, 0]


def test_kept_batch(prog):
    """batch_masses: no counting launch, rows = b * T_max, store = 0, cfrom = L; no m table of the context's own."""
    for bt in (P.Batch(LENS, NS, kept=True), P.Batch(LENS, NS, caps=[25, 12, 4], counted=[5, 0, 1], decoded=[6, 9, 0], ostats_done=[23, 2, 1], kept=True)):
        got = check(prog, every_kind(bt, FROMS, LAGS))
        for h, t, ds in got:
            assert h.mass_rows == 0 and h.word_rows == 3 * bt.T_max and t.count_gy == 0
            assert [(d.rows, d.store, d.cfrom) for d in ds] == [(b * bt.T_max, 0, L) for b, L in enumerate(LENS)]


def test_online_batch_before_its_first_observes(prog):
    """Every pass ends after its memsets but the predictive rows, which go on: row 0 needs no observe."""
    bt = P.Batch([0, 0, 0], NS, caps=[25, 12, 4])
    cases = every_kind(bt, (None, [0, 0, 0]), LAGS, n_traj=7)
    got = check(prog, cases)
    for (_, kind, kw), (h, t, ds) in zip(cases, got):
        assert bool(h.done) == (kind != "predictive"), kind
        d, e = kw.get("doubles", True), kw.get("entries", True)
        want = dict(stats=("stats_bytes", 3 * 88 * 8), online_stats=("stats_bytes", 3 * 88 * 8), traj_stats=("stats_bytes", 3 * 7 * 88 * 8),
                    smooth=("marg_bytes", 3 * 25 * 8 * 8 * d), smooth_lag=("marg_bytes", 3 * 2 * 8 * 8 * d), predictive=("marg_bytes", 3 * 2 * 8 * 8),
                    forecast=("marg_bytes", 3 * 6 * 8 * 8 * d), decode=("score_bytes", 3 * 8 * d), decode_lag=("score_bytes", 3 * 8 * d))[kind]
        assert getattr(h, want[0]) == want[1], kind
        assert h.traj_bytes == (3 * 7 * 7 * e if kind == "forecast" else 0) and h.path_bytes == (3 * 2 * e if kind == "decode_lag" else 0)
        if kind == "predictive":
            assert t.predictive_gy == 1 and t.count_gy == 0 and [x.cfrom for x in ds] == [0, 0, 0]


def test_length_zero_beside_a_live_problem(prog):
    for bt in (P.Batch([0, 7], [5, 3]), P.Batch([0, 7], [5, 3], caps=[3, 9], counted=[0, 2], decoded=[0, 7], ostats_done=[0, 3])):
        got = check(prog, every_kind(bt, (None, [0, 7], [0, 2]), LAGS))
        assert not any(h.done for h, _, _ in got)


def test_predictive_rows_nobody_owes(prog):
    """from = L + 1: nothing owed; everywhere: no launch."""
    bt = P.Batch(LENS, NS)
    a, b = check(prog, [(bt, "predictive", dict(frm=[24, 0, 2], n_rows=10)), (bt, "predictive", dict(frm=[24, 10, 2], n_rows=10))])
    assert a[1].predictive_gy == 3 and [d.cfrom for d in a[2]] == [23, 0, 1] and a[1].count_gy == 9
    assert not b[0].done and b[1].predictive_gy == 0 and [d.cfrom for d in b[2]] == [23, 9, 1] and b[1].count_gy == 0
    online = P.Batch(LENS, NS, caps=[25, 12, 4], counted=[5, 0, 1])
    check(prog, [(online, "predictive", dict(frm=f, n_rows=10)) for f in ([24, 0, 2], [24, 10, 2])])


@pytest.mark.parametrize("B,T,gy", [(1, 5, 5), (1024, 5, 5), (1025, 9, 8), (2, 5000, 4096)])
def test_count_grid(prog, B, T, gy):
    """gridDim.y = min(rows owed, max(8, ceil(8192 / B)))."""
    bt = P.Batch([T] * B, [2] * B)
    got = check(prog, [(bt, "smooth", dict(n_traj=1)), (bt, "stats", {}), (bt, "decode", {})])
    assert all(t.count_gy == gy for _, t, _ in got)
    assert got[1][1].stats_gx == got[2][1].decode_gx == (B + 3) // 4


def test_lag_grids_reach_their_limits(prog):
    """Plan arithmetic only: nothing of these sizes is allocated."""
    T = P.THREADS * 4096 + 300
    (_, t, _), (_, u, _), (_, v, _) = check(prog, [(P.Batch([T, 3], [1, 1]), "decode_lag", dict(lag=0, n_rows=T)),
                                                   (P.Batch([T - 557, 3], [1, 1]), "decode_lag", dict(lag=0, n_rows=T)),
                                                   (P.Batch([T, 3], [1, 1]), "decode_lag", dict(lag=T, n_rows=T))])
    assert (t.trace_gy, u.trace_gy, v.trace_gy) == (1 + 4096, 4096, 1)
    T = P.WAVES * 4096 + 7
    (_, t, _), (_, u, _) = check(prog, [(P.Batch([T, 3], [1, 1]), "smooth_lag", dict(lag=0, n_rows=T, n_traj=0)),
                                        (P.Batch([T - 12, 3], [1, 1]), "smooth_lag", dict(lag=0, n_rows=T, n_traj=0))])
    assert (t.lag_gy, u.lag_gy, t.smooth_gy) == (4096, 4095, 0) and t.lds_bytes == 64


@pytest.mark.parametrize("n_traj,tiles,stat_tiles", [(0, 0, 0), (1, 1, 1), (256, 1, 1), (257, 1, 2), (1025, 2, 5)])
def test_tile_counts(prog, n_traj, tiles, stat_tiles):
    bt = P.Batch(LENS, NS)
    s, f, ts, lg = check(prog, [(bt, "smooth", dict(n_traj=n_traj)), (bt, "forecast", dict(horizon=2, n_traj=n_traj)), (bt, "traj_stats", dict(n_traj=n_traj)),
                                (bt, "smooth_lag", dict(lag=2, n_rows=23, n_traj=n_traj))])
    assert s[1].smooth_gy == f[1].forecast_gy == 1 + tiles and ts[1].traj_stats_gy == stat_tiles
    assert lg[1].smooth_gy == (1 + tiles if n_traj else 0) and lg[1].lds_bytes == 3 * 64 and s[1].lds_bytes == 23 * 64


def test_the_arithmetic_lives_in_the_plan_header():
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    plan = open(os.path.join(CSRC, "batch_pass_plan.hpp")).read()
    assert '#include "batch_pass_plan.hpp"' in hip
    assert "std::max(mfrom, 1) - 1" not in hip and plan.count("std::max(mfrom, 1) - 1") == 1      # (the predictive rows' cfrom)
    incs = re.findall(r'#include\s*[<"]([^>"]+)[>"]', plan)
    assert sorted(incs) == ["algorithm", "cstddef", "cstdint"], "plain C++: no HIP, no kernel header, no context"
    assert "cpprob_hip_ctx" not in plan and "hip" not in re.sub(r"//[^\n]*", "", plan).lower()
