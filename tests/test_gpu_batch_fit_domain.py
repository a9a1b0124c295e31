"""The arithmetic of csrc/batch_scale.hpp on the device across its domain: table_log over the arguments the host measures it on
(tests/test_scale_ref_host.py's ARGS: every binary exponent range, the fold at sqrt(2), 1 +- 1e-3), scale_entry's division at
quotients whose last bit shows in the row, and scale_sigma's square root with the division before it and the logarithm behind it over
the same exponent range -- all through the public calls, array_equal on bits against tests/scale_ref.py, cpprob_amd.em.m_step and a
second context that BEGINS with the tables (the host's table_log against the device's).  The inputs are tests/fit_grid_cases.py's;
tests/test_fit_grid_cases_host.py proves that they reach what they claim.

B = 2006 problems of k = 8 states and one observe: 16048 states.  Nothing is run through the step kernel, so a row of -inf is harmless.
A fused multiply-add inside table_log changes its result at one argument in some 6000 and at none of those 16048: the sixty-four
sigmas of fit_grid_cases.fused_case (8 problems) are there to show a build that contracts it.

batch_retable_scaled_kernel and batch_mstep_scaled_kernel hold two of the three inlined copies of table_log on the device.  The third,
in batch_learn_scaled_kernel, takes the sigma of its own M-step (tau is internal): it cannot be driven at chosen arguments through the
public interface and is left to the ragged schedule of tests/test_gpu_batch_learn_scaled.py."""
import numpy as np
import pytest

import cpprob_amd as cp
import fit_grid_cases as F
import retable_ref as R
import scale_ref as S
from cpprob_amd import em
from test_gpu_batch_scale import _dev, _tables

pytestmark = pytest.mark.gpu

K, N = 8, 64


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the batch that BEGINS with the tables."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _retabled(engine, y, tables):
    """A scaled batch of one observe a problem begun with ordinary tables, then re-tabled on the device to `tables`."""
    B = len(y)
    obs = [y[b:b + 1] for b in range(B)]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=_tables(B, K, 5), keep_history=False, keep_masses=True)
    engine.batch_retable_device(_dev(tables[0]), _dev(tables[1]), _dev(y), sigmas=_dev(tables[2]))
    engine.sync()
    assert not engine.batch_retable_status().any() and engine.batch_retable_grid() == 1
    return obs


def _held(eng, B):
    """(rows [B, 8], words [B, 64], sigmas [B, 8], log_norms [B, 8]) as the device holds them."""
    rows, thr = zip(*[eng.batch_step_tables(b) for b in range(B)])
    sg, ln = zip(*[eng.batch_scales(b) for b in range(B)])
    return np.concatenate(rows), np.stack(thr), np.stack(sg), np.stack(ln)


def test_table_log_on_the_device_over_the_hosts_arguments(engine, ref_engine):
    sigmas = F.log_sigmas()
    B = sigmas.shape[0]
    means, trans, _ = _tables(B, K, 6)
    y = np.random.default_rng(7).uniform(-3.0, 7.0, B)
    obs = _retabled(engine, y, (means, trans, sigmas))
    rows, thr, sg, ln = _held(engine, B)
    want_ln = np.array([[S.log_norm(s) for s in row] for row in sigmas])
    assert np.array_equal(_bits(sg), _bits(sigmas))
    differ = _bits(ln) != _bits(want_ln)
    assert not differ.any(), "%d of %d log_norms differ, the first at sigma = %s" % (differ.sum(), differ.size, sigmas[differ][0].hex())
    want_rows = np.concatenate([S.rows(obs[b], means[b], sigmas[b], K) for b in range(B)])
    assert np.array_equal(_bits(rows), _bits(want_rows))
    assert all(np.array_equal(thr[b], R.thresholds(trans[b], K)) for b in range(0, B, 50))
    # the host route's table_log against the device's
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=(means, trans, sigmas), keep_history=False, keep_masses=True)
    for got, want in zip((rows, thr, sg, ln), _held(ref_engine, B)):
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    print("compared %d log_norms, %d row entries" % (ln.size, rows.size))


def test_table_log_on_the_device_where_a_fused_multiply_add_would_show(engine):
    """Sixty-four sigmas whose log_norm a contracted table_log changes (fit_grid_cases.fused_case; the 16048 arguments above hold
    none), through the re-table kernel's copy and, as sqrt(occ_yy / occ), through the M-step kernel's."""
    import torch
    v, sigmas = F.fused_case()
    B = sigmas.shape[0]
    means, trans, _ = _tables(B, K, 9)
    want = np.array([[S.log_norm(s) for s in row] for row in sigmas])
    _retabled(engine, np.zeros(B), (means, trans, sigmas))
    _, _, sg, ln = _held(engine, B)
    assert np.array_equal(_bits(sg), _bits(sigmas)) and np.array_equal(_bits(ln), _bits(want)), "re-table: %d of 64 log_norms differ" % np.sum(_bits(ln) != _bits(want))
    rec = np.zeros((B, R.RECORD))
    rec[:, :64], rec[:, 64:72], rec[:, 80:88] = 1.0, 1.0, v
    m, t, s, ln = _dev(means), _dev(trans), _dev(np.ones((B, K))), _dev(np.full((B, K), -7.0))
    engine.batch_mstep_device(_dev(rec), m, t, sigmas=s, sigma_floor=F.SIGMA_FLOOR, log_norms=ln)
    engine.sync()
    torch.cuda.synchronize()
    s, ln = s.cpu().numpy(), ln.cpu().numpy()
    assert np.array_equal(_bits(s), _bits(sigmas)) and np.array_equal(_bits(ln), _bits(want)), "M-step: %d of 64 log_norms differ" % np.sum(_bits(ln) != _bits(want))


def test_the_division_on_the_device_where_its_last_bit_shows(engine):
    y, means, sigmas = F.division_case()
    B = len(y)
    trans = _tables(B, K, 8)[1]
    obs = _retabled(engine, y, (means, trans, sigmas))
    rows = np.concatenate([engine.batch_step_tables(b)[0] for b in range(B)])
    want = np.concatenate([S.rows(obs[b], means[b], sigmas[b], K) for b in range(B)])
    differ = _bits(rows) != _bits(want)
    assert not differ.any(), "%d of %d entries differ, the first at y = %s, sigma = %s" % (
        differ.sum(), differ.size, np.broadcast_to(y[:, None], differ.shape)[differ][0].hex(), sigmas[differ][0].hex())
    print("compared %d row entries" % rows.size)


def test_the_scaled_mstep_kernel_over_the_exponent_range(engine):
    """batch_mstep_scaled_kernel's division, square root and logarithm at 16048 threads: 63 workgroups."""
    import torch
    rec, means, trans, sigmas = F.mstep_records()
    B = rec.shape[0]
    assert B * K == 16048 and (B * K + 255) // 256 == 63
    y = np.zeros(B)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [y[b:b + 1] for b in range(B)], N, tables=(means, trans, sigmas), keep_history=False, keep_masses=True)
    m, t, s, ln = _dev(means), _dev(trans), _dev(sigmas), _dev(np.full(sigmas.shape, -7.0))
    engine.batch_mstep_device(_dev(rec), m, t, sigmas=s, sigma_floor=F.SIGMA_FLOOR, log_norms=ln)
    engine.sync()
    torch.cuda.synchronize()
    m, t, s, ln = (x.cpu().numpy() for x in (m, t, s, ln))
    want = [S.m_step(rec[b], means[b], sigmas[b], np.full(K, -7.0), trans[b], K, F.SIGMA_FLOOR) for b in range(B)]
    wm, ws, wl, wt = (np.stack([w[i] for w in want]) for i in range(4))
    for got, ref, what in ((m, wm, "means"), (t, wt, "transition rows"), (s, ws, "sigmas")):
        differ = _bits(got) != _bits(ref)
        assert not differ.any(), "%s: %d of %d differ, the first in problem %d" % (what, differ.sum(), differ.size, np.argwhere(differ)[0][0])
    assert np.array_equal(ln, wl, equal_nan=True) and np.array_equal(_bits(ln)[~np.isnan(wl)], _bits(wl)[~np.isnan(wl)])
    assert np.isnan(wl).any() and (ws == F.SIGMA_FLOOR).any()
    hm, ht, hs = em.m_step(cp.capi.split_stats(rec), means, trans, sigmas, F.SIGMA_FLOOR)
    assert np.array_equal(_bits(hm), _bits(m)) and np.array_equal(_bits(ht), _bits(t)) and np.array_equal(_bits(hs), _bits(s))
    print("compared %d means, sigmas and log_norms, %d transition entries" % (m.size, t.size))
