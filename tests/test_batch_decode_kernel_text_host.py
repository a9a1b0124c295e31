"""batch_decode_forward_kernel and batch_decode_trace_kernel (csrc/batch_decode.hpp) as host code: the translation unit is formed here
from the text of csrc/batch_smooth.hpp and csrc/batch_decode.hpp (the former as tests/test_batch_smooth_kernel_text_host.py forms it,
the latter's include line naming that text), built against tests/host_kernels/batch_smooth_shim.hpp as a stand-alone program with g++
-O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_decode_main.cpp) and run
over grids from one workgroup for all problems to one a wavefront, and trace grids from one item a trip to several trips.  Every buffer
has exactly the size the host code hands the kernel; rows of the m table, the per-step table and the words no problem has reached are
NaN / 0xFFFFFFFF; the words, the v rows, the scores and the paths must equal tests/decode_ref.py's bit for bit.  Nothing is loaded
into python and nothing runs on a GPU.

The case file: a header of 15 int64 {magic, B, k, T_max, lp_stride, doubles of lp, rows of the m table (and words), 1: the full
decode, lag, n_rows, entries of the path output, gridDim.x of the forward launch, gridDim.y of the trace launch, 1: run the forward
launch, 1: run the trace launch}, then the descriptors, lp, lp0, the m table, the per-step table, the v rows and the words.  The
output: the words, the v rows [B][8], the scores [B], the path output int8."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import decode_ref as D
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b4445434f443031
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8"), ("rows", "<i8"), ("trows", "<i8"), ("cfrom", "<i4"), ("cto", "<i4"), ("lo", "<i4"), ("mfrom", "<i4")])
K_WAVES, K_THREADS = 4, 256
UNSET = 0xFFFFFFFF


def _texts():
    """(csrc/batch_smooth.hpp, csrc/batch_decode.hpp) with their textual changes; each must find its line exactly once."""
    smooth = open(os.path.join(CSRC, "batch_smooth.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert smooth.count(inc) == 1
    smooth = smooth.replace(inc, '#include "batch_smooth_shim.hpp"')
    lds = re.findall(r"^[ \t]*extern __shared__[^\n;]*\bs_mass\[\];", smooth, re.M)
    assert len(lds) == 1 and smooth.count("extern __shared__") == 1, lds
    smooth = smooth.replace(lds[0], "    double* s_mass = hostk::dynamic_lds();")
    dc = open(os.path.join(CSRC, "batch_decode.hpp")).read()
    inc = '#include "batch_smooth.hpp"'
    assert dc.count(inc) == 1 and dc.count("#include") == 1
    code = re.sub(r"//[^\n]*", "", dc)
    assert "extern" not in code and "atomic" not in code and "__shared__" not in code and "__syncthreads" not in code, "the decode kernels use no LDS, no barrier and no atomics"
    calls = re.findall(r"\b(\w*(?:log|exp)\w*)\s*\(", code)
    assert sorted(calls) == ["decode_log_table", "log", "log"], "the logarithms are the host's (decode_log_table): %s" % calls
    assert code.count("#pragma clang fp contract(off)") == 2
    return smooth, dc.replace(inc, '#include "batch_smooth_host.hpp"')


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_decode_host"))
    smooth, dc = _texts()
    open(os.path.join(d, "batch_smooth_host.hpp"), "w").write(smooth)
    open(os.path.join(d, "batch_decode_host.hpp"), "w").write(dc)
    so = O.build()
    exe = os.path.join(d, "batch_decode_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_decode_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(bt, lens, lo, v, words, forward, grid_x=1, trace=False, full=True, lag=0, frm=None, n_rows=0, grid_y=1):
        """(words, v rows [B, 8], scores [B], path output) of batch `bt` at the lengths reached `lens`, the forward pass from steps lo."""
        desc = bt.desc(lens, lo, frm)
        entries = int(sum(lens)) if full else bt.B * n_rows
        head = np.array([MAGIC, bt.B, bt.k, bt.T_max, bt.lp_stride, bt.lp.size, bt.n_rows, int(full), lag, n_rows, entries, grid_x, grid_y,
                         int(forward), int(trace)], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in ((desc, DESC), (bt.lp, np.float64), (np.array([bt.lp0]), np.float64), (bt.mass, np.float64), (bt.tab, np.float64),
                            (v, np.float64), (words, np.uint32)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        nw = 4 * bt.n_rows
        assert len(raw) == nw + 8 * 8 * bt.B + 8 * bt.B + entries
        return (np.frombuffer(raw[:nw], np.uint32).copy(), np.frombuffer(raw[nw:nw + 64 * bt.B], np.float64).reshape(bt.B, 8).copy(),
                np.frombuffer(raw[nw + 64 * bt.B:nw + 72 * bt.B], np.float64).copy(), np.frombuffer(raw[nw + 72 * bt.B:], np.int8).copy())
    return run


class Batch:
    """Problems of lengths Ts (capacities caps: an online batch's tables, addressed by capacity) with random states and table rows.
    Model HMM_TABLE: a table a problem, the second one's with a zero transition entry; HMM3: one table, and the entries 3 .. 7 of a
    table row hold what is no log-likelihood.  The m table, the per-step table and the words hold NaN / all ones wherever no problem
    has a row."""

    def __init__(self, Ts, ns, k, hmm3, seed, caps=None):
        rng = np.random.default_rng(seed)
        self.Ts, self.k, self.hmm3, self.B = list(Ts), k, hmm3, len(Ts)
        self.caps = list(caps) if caps else list(Ts)
        self.T_max = max(max(self.caps), 1)
        self.rows = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        self.n_rows = int(self.rows[-1])
        trans = rng.uniform(0.05, 1.0, (1 if hmm3 else self.B, k, k))
        if not hmm3 and self.B > 1:
            trans[1, 0, k - 1] = 0.0
        self.lp_stride = 0 if hmm3 else 64
        self.lp = np.full((trans.shape[0], 8, 8), -np.inf)
        self.lps = []
        for i, tr in enumerate(trans):
            lp, self.lp0 = D.log_table(R.transition_masses(tr))
            self.lps.append(lp)
            self.lp[i, :k, :k] = np.array(lp)
        self.mass = np.full((self.n_rows, 8), np.nan)
        self.tab = np.full((self.B, self.T_max, 8), np.nan)
        self.m, self.ll = [], []
        for b, (T, n) in enumerate(zip(self.Ts, ns)):
            v = rng.integers(0, k, (T, n))
            ll = -rng.uniform(0.0, 30.0, (T, k))
            m = R.filtering_masses(v, ll.tolist()) if T else []
            self.m.append(m)
            self.ll.append(ll.tolist())
            self.mass[self.rows[b]:self.rows[b] + T] = 0.0
            self.tab[b, :T] = 1e300                                  # (HMM3: exponentials and a maximum; never a log-likelihood)
            if T:
                self.mass[self.rows[b]:self.rows[b] + T, :k] = np.array(m, np.float64)
                self.tab[b, :T, :k] = ll

    def table(self, b):
        return self.lps[0 if self.hmm3 else b]

    def desc(self, lens, lo=None, frm=None):
        """batch_smooth_enqueue's descriptors at the lengths reached: lo the forward pass's first step, mfrom the first fixed-lag row."""
        d = np.zeros(self.B, DESC)
        at = 0
        for b, L in enumerate(lens):
            d[b] = (L, 1, 0, self.rows[b], at, L, L, 0 if lo is None else lo[b], 0 if frm is None else frm[b])
            at += L
        return d

    def fresh(self):
        return np.full((self.B, 8), np.nan), np.full(self.n_rows, UNSET, np.uint32)

    def want_words(self, lens):
        w = np.full(self.n_rows, UNSET, np.uint32)
        vs, sc = np.full((self.B, 8), np.nan), np.zeros(self.B)
        for b, L in enumerate(lens):
            if L:
                ww, v = D.forward(self.m[b][:L], self.ll[b][:L], self.table(b), self.lp0)
                w[self.rows[b]:self.rows[b] + L] = ww
                vs[b] = -np.inf
                vs[b, :self.k] = v
                sc[b] = max(v)
        return w, vs, sc

    def check_full(self, prog, lens, grid_x=1):
        v0, w0 = self.fresh()
        words, v, score, path = prog(self, lens, None, v0, w0, True, grid_x, trace=True, full=True)
        ww, wv, ws = self.want_words(lens)
        assert np.array_equal(words, ww), "words differ"
        assert np.array_equal(v, wv, equal_nan=True) and np.array_equal(score, ws)
        at = 0
        for b, L in enumerate(lens):
            wp, sc = D.decode(self.m[b][:L], self.ll[b][:L], self.table(b), self.lp0)
            assert np.array_equal(path[at:at + L], wp), "problem %d, length %d: paths differ" % (b, L)
            assert score[b] == sc
            at += L
        return words, v, path

    def check_lag(self, prog, lens, words, v, lag, grid_y, frm=None, n_rows=None):
        fr = [0] * self.B if frm is None else frm
        n_rows = max(max(L - f for L, f in zip(lens, fr)), 0) if n_rows is None else n_rows
        _, _, _, st = prog(self, lens, None, v, words, False, trace=True, full=False, lag=lag, frm=frm, n_rows=n_rows, grid_y=grid_y)
        st = st.reshape(self.B, n_rows)
        for b, L in enumerate(lens):
            want = D.decode_lag(words[self.rows[b]:self.rows[b] + L], lag, fr[b], n_rows)
            assert np.array_equal(st[b], want), "problem %d, length %d, lag %d, grid %d: fixed-lag rows differ" % (b, L, lag, grid_y)
        return st


TS = [0, 1, 2, 63, 64, 65, 130]
NS = [5, 3, 1, 70, 300, 9, 40]


@pytest.fixture(scope="module", params=["hmm3", "table2", "table5", "table8"])
def batch(request):
    if request.param == "hmm3":
        return Batch(TS, NS, 3, True, 5)
    k = int(request.param[5:])
    return Batch(TS, NS, k, False, 7 + k)


def test_full_decode_is_the_references(prog, batch):
    """Lengths across the 64-word staging chunk; seven problems on two workgroups' wavefronts (one left idle) and on one workgroup in
    two trips; the length-0 problem owns no entry and has score 0."""
    a = batch.check_full(prog, TS, grid_x=2)
    b = batch.check_full(prog, TS, grid_x=1)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    assert a[2].min() >= 0 and a[2].max() < batch.k


@pytest.mark.parametrize("B", [1, 5])
def test_batch_sizes_off_the_wavefronts(prog, B):
    bt = Batch([65, 2, 130, 1, 64][:B], [30, 1, 7, 2, 64][:B], 5, False, 31 + B)
    bt.check_full(prog, bt.Ts, grid_x=1)
    bt.check_full(prog, bt.Ts, grid_x=(B + K_WAVES - 1) // K_WAVES)


def test_fixed_lag_rows_on_every_grid(prog, batch):
    """lag in {0, 1, 3, L}; gridDim.y = 2: every lane item in one trip."""
    words, v, path = batch.check_full(prog, TS)
    at = np.concatenate([[0], np.cumsum(TS)])
    for lag in (0, 1, 3, 130):
        st = batch.check_lag(prog, TS, words, v, lag, 2)
        for b, L in enumerate(TS):
            tail = [t for t in range(L) if t + lag >= L - 1]
            assert np.array_equal(st[b, tail], path[at[b]:at[b + 1]][tail]), "the rows whose end is L - 1 are the full decode's"
            assert np.all(st[b, L:] == -1)
    frm = [0, 1, 1, 60, 3, 65, 100]                            # (problems 1 and 5: from = L, no row)
    for lag in (0, 3):
        st = batch.check_lag(prog, TS, words, v, lag, 3, frm=frm, n_rows=70)
        assert np.all(st[1] == -1) and np.all(st[5] == -1)


def test_trace_items_in_several_trips(prog):
    """A problem of 600 steps: 599 lane items at lag 0 take three trips of one workgroup, two of two, one of three."""
    bt = Batch([600, 3], [20, 4], 3, False, 77)
    words, v, _ = bt.check_full(prog, bt.Ts)
    for gy in (2, 3, 4):
        bt.check_lag(prog, bt.Ts, words, v, 0, gy)
    bt.check_lag(prog, bt.Ts, words, v, 70, 2)
    bt.check_lag(prog, bt.Ts, words, v, 600, 1)               # (no lane item: the full decode's rows)


def test_forward_pass_at_every_watermark(prog):
    """A 5-step stream in tables addressed by capacity: the forward pass resumed at every watermark gives the one-shot words, v rows
    and scores; a problem still at length 0 sits between two that are not."""
    bt = Batch([5, 5, 5], [70, 1, 300], 5, False, 11, caps=[7, 6, 9])
    one = bt.check_full(prog, [5, 5, 5])
    for cut in range(0, 6):
        v, words = bt.fresh()
        lens = [cut, 0, min(cut, 2)]
        if any(lens):
            words, v, sc, _ = prog(bt, lens, None, v, words, True)
            ww, wv, ws = bt.want_words(lens)
            assert np.array_equal(words, ww) and np.array_equal(sc, ws)
        words, v, sc, path = prog(bt, [5, 5, 5], lens, v, words, True, trace=True, full=True)
        assert np.array_equal(words, one[0]) and np.array_equal(v, one[1]) and np.array_equal(path, one[2])
    # one observe at a time
    v, words = bt.fresh()
    for L in range(1, 6):
        words, v, sc, path = prog(bt, [L, L, L], [L - 1] * 3, v, words, True, trace=True, full=True)
        assert np.array_equal(sc, bt.want_words([L, L, L])[2])
    assert np.array_equal(words, one[0]) and np.array_equal(v, one[1]) and np.array_equal(path, one[2])
    # nothing new: the saved rows give the score again
    w2, v2, sc2, p2 = prog(bt, [5, 5, 5], [5, 5, 5], v, words, True, trace=True, full=True)
    assert np.array_equal(w2, words) and np.array_equal(v2, v) and np.array_equal(sc2, sc) and np.array_equal(p2, path)


def test_zero_entry_is_never_taken(prog):
    """Table 1 has P[0][k-1] = 0: no finite path of problem 1 steps from state 0 to state k - 1."""
    bt = Batch([40, 40, 40], [50, 50, 50], 5, False, 21)
    assert bt.lps[1][0][4] == -math.inf
    _, v, path = bt.check_full(prog, bt.Ts)
    p = path[40:80]
    assert max(v[1]) > -math.inf and not np.any((p[:-1] == 0) & (p[1:] == 4))


def test_forward_pass_resumes_across_chunk_borders(prog):
    """A 150-step stream fed as 63 + 1 + 1 + 63 + 1 + 21 into tables addressed by capacity, decoded after every advance: the forward
    pass resumes from the saved v row at 63, 64, 65, 128 and 129, and row 0 of the traceback walks chunks whose words were written by
    different launches.  Problem 1 is never fed; problem 2's stream ends at 128."""
    bt = Batch([150, 5, 128], [70, 1, 30], 5, False, 13, caps=[150, 9, 130])
    v, words = bt.fresh()
    lens, resumed = [0, 0, 0], []
    for dT in (63, 1, 1, 63, 1, 21):
        lo, lens = lens, [min(lens[0] + dT, 150), 0, min(lens[2] + dT, 128)]
        resumed.append(lo[0])
        words, v, sc, path = prog(bt, lens, lo, v, words, True, grid_x=1, trace=True, full=True)
        ww, wv, ws = bt.want_words(lens)
        assert np.array_equal(words, ww), "lengths %s: words differ" % lens
        assert np.array_equal(v[[0, 2]], wv[[0, 2]]) and np.array_equal(sc, ws), "lengths %s" % lens
        at = 0
        for b, L in enumerate(lens):
            wp, _ = D.decode(bt.m[b][:L], bt.ll[b][:L], bt.table(b), bt.lp0)
            assert np.array_equal(path[at:at + L], wp), "problem %d resumed at %d, length %d: paths differ" % (b, lo[b], L)
            at += L
        for gy in (2, 3):
            bt.check_lag(prog, lens, words, v, 3, gy)
    assert resumed == [0, 63, 64, 65, 128, 129] and lens == [150, 0, 128]
    one = bt.check_full(prog, lens)
    assert np.array_equal(words, one[0]) and np.array_equal(v[[0, 2]], one[1][[0, 2]]) and np.array_equal(path, one[2])
    carried = [int(x) for x in path[:150][[149 - 64, 149 - 128]]]
    assert any(carried), "every state carried across a chunk border is zero: choose another seed"
