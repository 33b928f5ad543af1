"""
CPU tests of tests/solve_cases.py and of csrc/solve_core.h on its cells (no kernel launched): the directed set holds what
it promises, measured with the reference alone, and the scalar solve compiled for the host answers as the oracle does on
every directed cell, every boundary cell and every level of the adversarial tables.  The GPU tests
(test_gpu_solve_reference.py) then show the device only cases its host twin already agrees on.
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import scipy.stats

import solve_cases as SC
from conftest import ROOT
from kbbq import _solve

x87 = pytest.mark.skipif(np.finfo(np.longdouble).nmant != 63, reason='np.longdouble is not x87 extended here')


@pytest.fixture(scope='module')
def solver(tmp_path_factory):
    """solve_cell of csrc/solve_core.h as a host program (the recipe of test_solve_core_host.py); the gammaln term is the
    caller's."""
    exe = str(tmp_path_factory.mktemp('native') / 'solve_check')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-fsanitize=undefined', '-fno-sanitize-recover=undefined', '-o', exe,
                           os.path.join(ROOT, 'tests', 'native', 'solve_check.cpp')])

    def run(prior_q, errs, total, comb):
        shape = np.shape(prior_q)
        rec = np.empty(int(np.prod(shape)), dtype=[('p', '<i8'), ('e', '<i8'), ('t', '<i8'), ('c', '<f8')])
        rec['p'], rec['e'], rec['t'], rec['c'] = (np.asarray(x).ravel() for x in (prior_q, errs, total, comb))
        blob = struct.pack('<q', rec.size) + _solve.model_consts().tobytes() + rec.tobytes()
        out = subprocess.run([exe], input=blob, capture_output=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return (np.frombuffer(out.stdout, dtype=np.int64) - rec['p']).reshape(shape)
    return run


@x87
def test_directed_cells_meet_their_floors():
    """Measured with the reference alone (NumPy, SciPy, the oracle): enough cells per prior, enough cells of every kind a wrong
    kernel would answer differently, and the NumPy statement of logpmf the kinds are derived from is SciPy's bit for bit."""
    d = SC.directed_cells()
    f = SC.floors(d)
    print('directed cells:', f)
    assert np.all((0 <= d.errs) & (d.errs <= d.total) & (d.total < SC.MAX_TOTAL))
    assert np.unique(np.stack([d.prior_q, d.errs, d.total]), axis=1).shape[1] == d.prior_q.size
    assert f['min_per_prior'] >= 16
    assert f['ties'] >= 10 and f['fused'] >= 25 and f['assoc'] >= 25 and f['double_add'] >= 1
    assert f['last_max'] == f['ties']
    assert np.array_equal(d.ref - d.prior_q, d.dq)                   # the NumPy restatement answers as the oracle does
    ll, _, _ = SC.loglike(d.errs, d.total)
    p = SC.O.q_to_p(np.arange(SC.NQ)).astype(np.float64)
    with np.errstate(all='ignore'):
        want = scipy.stats.binom.logpmf(d.errs + 1, d.total + 2, p[:, None])
    assert np.array_equal(ll.view(np.uint64), want.view(np.uint64))


@x87
def test_solve_core_on_directed_cells(solver):
    d = SC.directed_cells()
    got = solver(d.prior_q, d.errs, d.total, _solve.combiln(d.errs, d.total))
    bad = np.flatnonzero(got != d.dq)
    assert bad.size == 0, [(int(d.prior_q[i]), int(d.errs[i]), int(d.total[i]), int(got[i]), int(d.dq[i]),
                            [k for k in SC.KINDS if getattr(d, k)[i]]) for i in bad[:10]]


@x87
def test_solve_core_on_boundary_cells(solver):
    """k == n (errs == total + 1) lies inside the support: candidate 0's term is xlog1py(0, -1) = 0, not 0 * -inf."""
    b = SC.boundary_cells()
    assert b.prior_q.size == 567 and np.any(b.errs == b.total + 1) and np.any(b.errs == -1) and np.any(b.total == -2)
    got = solver(b.prior_q, b.errs, b.total, SC.comb_scipy(b.errs, b.total))
    bad = np.flatnonzero(got != b.dq)
    assert bad.size == 0, [(int(b.prior_q[i]), int(b.errs[i]), int(b.total[i]), int(got[i]), int(b.dq[i])) for i in bad[:10]]
    at_edge = (b.errs == b.total + 1) & (b.total >= -2)
    assert np.any(b.dq[at_edge] != -b.prior_q[at_edge])             # the edge is decided by more than "candidate 0"


@x87
def test_solve_core_level_by_level_on_adversarial_tables(solver):
    base = SC.tables(3, 66, 1)
    for t in (base, SC.with_dinuc(base, SC.directed_cells()), SC.with_dinuc(base, SC.boundary_cells())):
        meanq, rg_e, rg_t, q_e, q_t, p_e, p_t, d_e, d_t = t.vectors
        rgdq, qdq, posdq, dinucdq = t.dqs
        assert np.array_equal(solver(meanq, rg_e, rg_t, SC.comb_scipy(rg_e, rg_t)), rgdq)
        prior1 = np.broadcast_to((meanq + rgdq)[:, None], q_t.shape)
        assert np.array_equal(solver(prior1, q_e, q_t, SC.comb_scipy(q_e, q_t)), qdq)
        prior2 = np.broadcast_to(t.prior2[..., None], p_t.shape)
        assert np.array_equal(solver(prior2, p_e, p_t, SC.comb_scipy(p_e, p_t)), posdq)
        prior3 = np.broadcast_to(t.prior2[..., None], d_t.shape)
        assert np.array_equal(solver(prior3, d_e, d_t, SC.comb_scipy(d_e, d_t)), dinucdq[..., :16])
        assert not dinucdq[..., 16].any()


@x87
def test_tables_reference_is_independent_and_agrees_with_the_product():
    """tables() builds meanq in `decimal` and the marginals by NumPy sums; the product's host route (kbbq._solve: longdouble
    meanq, native marginals) must give the same vectors -- two derivations, one answer."""
    for R, S2 in ((1, 2), (3, 66), (2, 130)):
        t = SC.tables(R, S2, 1)
        aux, q_e, q_t, rg_e, rg_t = _solve.solve_prep(t.flat, R, S2)
        for got, want in zip((_solve.meanq_from_q_total(q_t), rg_e, rg_t, q_e, q_t), t.vectors):
            assert np.array_equal(got, want)
        assert np.all((q_t != 0).sum(axis=1) >= 2)


@x87
def test_with_dinuc_places_directed_cells_by_prior():
    d = SC.directed_cells()
    base = SC.tables(3, 4, 1)
    t = SC.with_dinuc(base, d)
    assert np.array_equal(d.prior_q[t.placed], np.broadcast_to(base.prior2[..., None], t.placed.shape))
    assert np.array_equal(t.dqs[3][..., :16], d.dq[t.placed])         # the table's reference is the cells' own
    for a, b in zip(t.dqs[:3], base.dqs[:3]):
        assert np.array_equal(a, b)
