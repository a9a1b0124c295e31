"""What the library's host code decides for one batch pass before it touches the device (csrc/batch_pass_plan.hpp, run by
batch_smooth_enqueue), stated in plain Python one pass after another: the bytes of the output memsets, whether the call ends after
them, the rows of the m table and of the word table, the problems' descriptors and every grid.  tests/test_batch_pass_plan_host.py
compares the header, built as a host program, with this for equality.

A batch: the lengths reached, the particle counts and the store offsets; an online batch (caps is not None) also has capacities and
the watermarks counted (rows of the m table), decoded (step words) and ostats_done (steps in tau); kept: the run left the m table
in the workspace, rows by T_max.  A pass's outputs are named by presence alone: `doubles` (the marginals, the predictive rows, or a
decode's scores) and `entries` (the trajectories, or a decode's path)."""
from collections import namedtuple

KINDS = ("smooth", "smooth_lag", "stats", "traj_stats", "online_stats", "forecast", "predictive", "decode", "decode_lag")
THREADS, WAVES, TILE, TRAJ_STATS_TILE, STATS = 256, 4, 1024, 256, 88
MAX_T, LDS_MAX, COUNT_GROUPS, LAG_GRID_MAX, PREDICTIVE_GRID_MAX, TRACE_GRID_MAX = 1 << 24, 32768, 8192, 4096, 4096, 4096

Head = namedtuple("Head", "marg_rows marg_bytes stats_bytes traj_bytes score_bytes path_bytes mass_rows word_rows done")
Tail = namedtuple("Tail", "fresh lag lds_bytes count_gy lag_gy smooth_gy stats_gx traj_stats_gy forecast_gy predictive_gy decode_gx trace_gy")
Desc = namedtuple("Desc", "T n store rows trows cfrom cto lo mfrom")


class Batch:
    def __init__(self, lens, ns, caps=None, counted=None, decoded=None, ostats_done=None, kept=False, T_max=None, spp=8):
        self.lens, self.ns, self.B = list(lens), list(ns), len(lens)
        self.online, self.kept, self.spp = caps is not None, kept, spp
        self.caps = list(caps) if self.online else [0] * self.B
        sizes = self.caps if self.online else self.lens
        self.store = [sum(t * n for t, n in zip(sizes[:b], self.ns[:b])) for b in range(self.B)]
        self.counted = list(counted) if counted else [0] * self.B
        self.decoded = list(decoded) if decoded else [0] * self.B
        self.ostats_done = list(ostats_done) if ostats_done else [0] * self.B
        self.T_max = T_max if T_max is not None else max(max(sizes), 1)
        self.reached = sum(self.lens)


def ceil_div(a, b):
    return (a + b - 1) // b


def _tables(bt):
    """(rows of the context's own m table, rows of the word table): by capacity where the batch is online; a kept batch has its m
    table in the workspace, [B][T_max], and none of the context's."""
    rows = sum(bt.caps) if bt.online else bt.reached
    return (0, bt.B * bt.T_max) if bt.kept else (rows, rows)


def _describe(bt, W, mfrom, cfrom_run, lo, trows=None):
    """The descriptors: a problem's first row of the m table is the capacities (online) or lengths before it, its first row of
    trajectory output the windows W before it; the rows the counting pass owes start at the watermark (online), at L (kept: none)
    or where this call first reads (a run batch keeps nothing: cfrom_run)."""
    out, at, at_traj = [], 0, 0
    for b, L in enumerate(bt.lens):
        rows, store = at, bt.store[b]
        if bt.kept:
            rows, store, cfrom = b * bt.T_max, 0, L
        elif bt.online:
            cfrom = bt.counted[b]
        else:
            cfrom = cfrom_run[b]
        out.append(Desc(L, bt.ns[b], store, rows, at_traj if trows is None else trows[b], cfrom, L, lo[b], mfrom[b]))
        at += bt.caps[b] if bt.online else L
        at_traj += W[b]
    return out


def _count_gy(bt, desc):
    owed = max(d.cto - d.cfrom for d in desc)
    return 0 if bt.kept or owed <= 0 else min(owed, max(8, ceil_div(COUNT_GROUPS, bt.B)))


def _tail(bt, desc, W, **grids):
    t = dict.fromkeys(Tail._fields, 0)
    t.update(lds_bytes=min(max(W) * 64, LDS_MAX), count_gy=_count_gy(bt, desc))
    t.update(grids)
    return Tail(**t)


def _head(bt, done, marg_rows, **sizes):
    mass_rows, word_rows = _tables(bt)
    h = dict.fromkeys(Head._fields, 0)
    h.update(marg_rows=marg_rows, mass_rows=mass_rows, word_rows=word_rows, done=int(done))
    h.update(sizes)
    return Head(**h)


def _tiles(n_traj, with_traj):
    return ceil_div(n_traj, TILE) if with_traj else 0


def smooth(bt, n_traj, doubles, entries):
    with_traj = bool(entries and n_traj)
    head = _head(bt, bt.reached == 0 or not (doubles or with_traj), bt.T_max, marg_bytes=bt.B * bt.T_max * bt.spp * 8 if doubles else 0)
    if head.done:
        return head, None, None
    zero = [0] * bt.B
    desc = _describe(bt, bt.lens, zero, zero, zero)
    return head, _tail(bt, desc, bt.lens, smooth_gy=1 + _tiles(n_traj, with_traj)), desc


def smooth_lag(bt, lag, frm, n_rows, n_traj, doubles, entries):
    with_traj = bool(entries and n_traj)
    head = _head(bt, bt.reached == 0 or not (doubles or with_traj), n_rows, marg_bytes=bt.B * n_rows * bt.spp * 8 if doubles else 0)
    if head.done:
        return head, None, None
    mfrom = list(frm) if frm is not None else [0] * bt.B
    W = [min(lag + 1, L) for L in bt.lens]
    lo = [L - w for L, w in zip(bt.lens, W)]
    # a run batch counts from the first row either output reads: the marginals' from, the window's start
    cfrom = [min(f if doubles else L, s if with_traj else L) for L, f, s in zip(bt.lens, mfrom, lo)]
    desc = _describe(bt, W, mfrom, cfrom, lo)
    items = max([max(1, L - f - lag) for L, f in zip(bt.lens, mfrom) if f < L], default=0)
    lag_gy = min(ceil_div(items, WAVES), LAG_GRID_MAX) if doubles and items > 0 else 0
    return head, _tail(bt, desc, W, lag=lag, lag_gy=lag_gy, smooth_gy=1 + _tiles(n_traj, True) if with_traj else 0), desc


def _full_walk(bt):
    zero = [0] * bt.B
    return _describe(bt, bt.lens, zero, zero, zero)


def stats(bt):
    head = _head(bt, bt.reached == 0, bt.T_max, stats_bytes=bt.B * STATS * 8 if bt.reached == 0 else 0)
    if head.done:
        return head, None, None
    desc = _full_walk(bt)
    return head, _tail(bt, desc, bt.lens, stats_gx=ceil_div(bt.B, WAVES)), desc


def traj_stats(bt, n_traj):
    head = _head(bt, bt.reached == 0, bt.T_max, stats_bytes=bt.B * n_traj * STATS * 8 if bt.reached == 0 else 0)
    if head.done:
        return head, None, None
    desc = _full_walk(bt)
    return head, _tail(bt, desc, bt.lens, traj_stats_gy=ceil_div(n_traj, TRAJ_STATS_TILE)), desc


def online_stats(bt):
    head = _head(bt, bt.reached == 0, bt.T_max, stats_bytes=bt.B * STATS * 8 if bt.reached == 0 else 0)
    if head.done:
        return head, None, None
    # lo: the first step to consume; trows: its observe among the fresh ones, packed
    lo = [min(d, L) for d, L in zip(bt.ostats_done, bt.lens)]
    fresh = [L - s for L, s in zip(bt.lens, lo)]
    trows = [sum(fresh[:b]) for b in range(bt.B)]
    zero = [0] * bt.B
    desc = _describe(bt, bt.lens, zero, zero, lo, trows)
    return head, _tail(bt, desc, bt.lens, fresh=sum(fresh), stats_gx=ceil_div(bt.B, WAVES)), desc


def forecast(bt, horizon, n_traj, doubles, entries):
    with_traj = bool(entries and n_traj)
    head = _head(bt, bt.reached == 0 or not (doubles or with_traj), horizon, marg_bytes=bt.B * horizon * bt.spp * 8 if doubles else 0,
                 traj_bytes=bt.B * (horizon + 1) * n_traj if bt.reached == 0 and with_traj else 0)
    if head.done:
        return head, None, None
    zero = [0] * bt.B
    desc = _describe(bt, bt.lens, zero, [max(L - 1, 0) for L in bt.lens], zero)          # (a run batch counts row L - 1 only)
    return head, _tail(bt, desc, bt.lens, forecast_gy=1 + _tiles(n_traj, with_traj)), desc


def predictive(bt, frm, n_rows, doubles):
    head = _head(bt, not doubles, n_rows, marg_bytes=bt.B * n_rows * bt.spp * 8 if doubles else 0)     # (row 0 needs no observe: it goes on at length 0)
    if head.done:
        return head, None, None
    mfrom = list(frm) if frm is not None else [0] * bt.B
    zero = [0] * bt.B
    # row r reads row r - 1 of the m table: a run batch counts rows max(from, 1) - 1 .. L - 1
    desc = _describe(bt, bt.lens, mfrom, [min(max(f, 1) - 1, L) for f, L in zip(mfrom, bt.lens)], zero)
    owed = max(L + 1 - f for L, f in zip(bt.lens, mfrom))
    return head, _tail(bt, desc, bt.lens, predictive_gy=min(ceil_div(owed, WAVES), PREDICTIVE_GRID_MAX) if owed > 0 else 0), desc


def _decode_lo(bt):
    return [min(d, L) if bt.online else 0 for d, L in zip(bt.decoded, bt.lens)]         # the forward pass's first step


def decode(bt, doubles, entries):
    head = _head(bt, bt.reached == 0, bt.T_max, score_bytes=bt.B * 8 if doubles else 0)
    if head.done:
        return head, None, None
    zero = [0] * bt.B
    desc = _describe(bt, bt.lens, zero, zero, _decode_lo(bt))
    return head, _tail(bt, desc, bt.lens, decode_gx=ceil_div(bt.B, WAVES), trace_gy=1 if entries else 0), desc


def decode_lag(bt, lag, frm, n_rows, doubles, entries):
    head = _head(bt, bt.reached == 0, bt.T_max, score_bytes=bt.B * 8 if doubles else 0, path_bytes=bt.B * n_rows if entries else 0)
    if head.done:
        return head, None, None
    mfrom = list(frm) if frm is not None else [0] * bt.B
    lag = min(lag, MAX_T)
    desc = _describe(bt, bt.lens, mfrom, [0] * bt.B, _decode_lo(bt))
    # row 0 of the trace grid: the item of end L - 1; the ends before it a lane each
    lane_items = max([L - 1 - f - lag for L, f in zip(bt.lens, mfrom)] + [0])
    trace_gy = 1 + min(ceil_div(lane_items, THREADS), TRACE_GRID_MAX) if entries else 0
    return head, _tail(bt, desc, bt.lens, lag=lag, decode_gx=ceil_div(bt.B, WAVES), trace_gy=trace_gy), desc


def plan(bt, kind, lag=0, frm=None, n_rows=0, horizon=0, n_traj=0, doubles=True, entries=True):
    """(Head, Tail, [Desc]) of pass `kind`; Tail and the descriptors are None where the call ends after its memsets."""
    if kind == "smooth":
        return smooth(bt, n_traj, doubles, entries)
    if kind == "smooth_lag":
        return smooth_lag(bt, lag, frm, n_rows, n_traj, doubles, entries)
    if kind == "stats":
        return stats(bt)
    if kind == "traj_stats":
        return traj_stats(bt, n_traj)
    if kind == "online_stats":
        return online_stats(bt)
    if kind == "forecast":
        return forecast(bt, horizon, n_traj, doubles, entries)
    if kind == "predictive":
        return predictive(bt, frm, n_rows, doubles)
    if kind == "decode":
        return decode(bt, doubles, entries)
    assert kind == "decode_lag", kind
    return decode_lag(bt, lag, frm, n_rows, doubles, entries)
