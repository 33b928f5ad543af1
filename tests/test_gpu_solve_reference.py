"""
GPU tests (-m gpu) of the model solve (K3) against the reference itself.  The product runs the wave form of the cell solve
(solve_cell_wave in csrc/kbbq_solve_kernels.h: one lane per candidate, a butterfly over an integer key of the 80-bit sum),
through dev.solve (gammaln terms and meanq from the host) and dev.solve_lut (everything on the device).  Here both routes,
and the scalar kernels behind compare_reads.gatk_delta_q, are compared with tests/solve_cases.py -- NumPy sums, `decimal`
and the oracle's SciPy / longdouble arithmetic -- never with each other: on adversarial tables at the widths where the
kernels change path, on cells where one rounding or the first-maximum rule decides the answer, and at the edges of the
binomial's support.  test_solve_cases_host.py shows the host twin of the arithmetic agrees on every one of these cells.
"""
import numpy as np
import pytest

import solve_cases as SC

pytestmark = pytest.mark.gpu

DIRECTED_SEED = 4              # tables(3, 4, seed) with the most distinct priors among seeds 1..8 (32), chosen on the CPU


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from kbbq import _device
    ctx = _device.context()
    assert 'gfx950' in ctx.name
    return _device


def _upload(dev, t):
    import torch
    tb = dev.Tables(t.R, t.S2)
    tb.buf.copy_(torch.from_numpy(t.flat.copy()))
    return tb


def _clear_status(dev):
    from kbbq import _native as N
    try:
        dev.context().status()
    except N.KbbqHipError:
        pass


def _differences(got, want, t):
    """The first few cells of the dinucleotide / cycle tables that differ, with their prior and counts, for the failure message."""
    out = []
    for name, g, w, e, n in (('pos', got[2], want[2], t.vectors[5], t.vectors[6]), ('dinuc', got[3][..., :16], want[3][..., :16], t.vectors[7], t.vectors[8])):
        for r, q, x in np.argwhere(g != w)[:6]:
            out.append((name, int(r), int(q), int(x), 'prior', int(t.prior2[r, q]), 'errs', int(e[r, q, x]), 'total', int(n[r, q, x]),
                        'got', int(g[r, q, x]), 'want', int(w[r, q, x])))
    return out


def _check_both_routes(dev, t):
    """dev.solve and dev.solve_lut on the tables `t`, each against t's reference: vectors, delta tables, the LUT blob byte for
    byte, and -- for solve_lut -- that the kernel decided meanq itself."""
    from kbbq import _native as N
    want_lut, want_shape = dev.build_lut(t.vectors[0], *t.dqs)
    tb = _upload(dev, t)
    _clear_status(dev)
    lut, shape, vectors, dqs = dev.solve(tb, want_dq=True)
    for got, want in zip(vectors, t.vectors):
        assert np.array_equal(got, want)
    assert all(np.array_equal(g, w) for g, w in zip(dqs, t.dqs)), _differences(dqs, t.dqs, t)
    assert shape[:3] == want_shape[:3]
    assert np.array_equal(lut.cpu().numpy(), want_lut)
    # the all-device route: no host pass behind it, and no meanq handed back to the host
    assert dev.device_logtab() is not None
    _clear_status(dev)
    lut2, shape2 = dev.solve_lut(tb)
    got2 = lut2.cpu().numpy()
    assert np.array_equal(got2, want_lut), _lut_differences(got2, want_lut, t)
    assert shape2 == want_shape
    ctx = dev.context()
    _clear_status(dev)
    dev.solve_lut(tb, check=False)
    if want_shape[3] == N.APPLY_FAST:
        ctx.status()                                   # raises nothing: meanq decided by the kernel, LUT usable as it is
    else:
        # the reference LUT itself needs the checked apply kernel (a cycle + context sum can leave 0..255): that, and
        # nothing about meanq (which the status word reports first), is what the kernels must say
        with pytest.raises(N.LutNeedsCheckedApply):
            ctx.status()


def _lut_differences(got, want, t):
    """Where two blobs differ, as (read group, quality, column) of the canonical int16 rows when the difference lies there."""
    from kbbq import _native as N
    n16 = np.flatnonzero(got != want)
    if n16.size == 0:
        return []
    rows, rs = t.R * SC.NQ, N.load().kbbq_lut_row_stride(t.S2)
    g16, w16 = got.view(np.int16), want.view(np.int16)
    out = []
    for i in np.flatnonzero(g16[:rows * rs] != w16[:rows * rs])[:8]:
        cell, col = divmod(int(i), rs)
        out.append((cell // SC.NQ, cell % SC.NQ, col, 'got', int(g16[i]), 'want', int(w16[i])))
    return out or [('bytes', n16[:8].tolist())]


def _stride_S2(dev):
    """(8, S2): the smallest even S2 at which k3_level_c's grid strides -- more cells than the 128 waves per compute unit
    it launches (80 at 256 compute units)."""
    cus = dev.context().compute_units
    S2 = 2
    while 8 * SC.NQ * (S2 + 16) <= 128 * cus:
        S2 += 2
    return S2


@pytest.mark.parametrize('R,S2', [(1, 2), (1, 62), (3, 66), (2, 130), (8, None)])
def test_fused_solve_both_routes_against_the_reference(dev, R, S2):
    """Adversarial tables (empty cells, errs == total, tiny cells, counts to 2e10).  S2 = 2 puts the boundary between cycle and
    dinucleotide cells inside a workgroup; 62, 66 and 130 lie around the 64-lane marginal loop; (8, S2) makes the grid stride."""
    if S2 is None:
        S2 = _stride_S2(dev)
        assert 8 * SC.NQ * (S2 + 16) > 128 * dev.context().compute_units >= 8 * SC.NQ * (S2 + 14)
    _check_both_routes(dev, SC.tables(R, S2, 1))


def test_fused_solve_on_directed_cells(dev):
    """The dinucleotide table filled with cells where rounding or the tie-break decides: a final add in double, a fused
    multiply-add, the other association of the sum or a last-maximum rule in the wave form would each change an answer."""
    d = SC.directed_cells()
    base = SC.tables(3, 4, DIRECTED_SEED)
    t = SC.with_dinuc(base, d)
    placed = t.placed.ravel()
    assert np.unique(base.prior2).size >= 20
    assert d.tie[placed].sum() >= 5 and d.fused[placed].sum() >= 10 and d.assoc[placed].sum() >= 10
    assert np.array_equal(t.dqs[3][..., :16].ravel(), d.dq[placed])
    _check_both_routes(dev, t)


def test_fused_solve_on_boundary_cells(dev):
    """The edges of the binomial's support in the dinucleotide table: outside it every candidate ties and the answer is
    candidate 0; k == n (errs == total + 1) and k == 0 lie inside it.  lgam_combiln answers NaN outside the support and
    passes gammaln only arguments >= 1 inside it."""
    b = SC.boundary_cells()
    t = SC.with_dinuc(SC.tables(1, 2, 1), b)
    e, n = t.vectors[7], t.vectors[8]
    edge = e == n + 1
    assert edge.sum() >= 40 and np.any((t.dqs[3][..., :16] + t.prior2[..., None])[edge] != 0)
    assert np.any(e == -1) and np.any(n < -2) and np.any(e > n + 1)
    _check_both_routes(dev, t)


@pytest.mark.parametrize('as_float', [False, True])
def test_scalar_kernels_on_directed_and_boundary_cells(dev, oracle, as_float):
    """compare_reads.gatk_delta_q (k3_delta_q; with a float64 prior k3_posterior_q) on every directed and boundary cell."""
    from kbbq import compare_reads
    d, b = SC.directed_cells(), SC.boundary_cells()
    pq = np.concatenate([d.prior_q, b.prior_q])
    errs, total = np.concatenate([d.errs, b.errs]), np.concatenate([d.total, b.total])
    want = np.concatenate([d.dq, b.dq])
    if as_float:
        pq = pq.astype(np.float64)
        want_f = oracle.gatk_delta_q(pq, errs, total)
        assert want_f.dtype == np.float64 and np.array_equal(want_f, want)
        want = want_f
    got = compare_reads.gatk_delta_q(pq, errs, total)
    assert got.dtype == want.dtype
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(pq[i], int(errs[i]), int(total[i]), got[i], want[i]) for i in bad[:10]]


def test_solve_lut_reuses_its_buffer(dev):
    """solve_lut(reuse=True) hands out the buffer it keeps per shape: after tables A, tables B of the same shape must leave
    B's reference blob in it, byte for byte -- nothing of A's survives."""
    a, b = SC.tables(3, 66, 1), SC.tables(3, 66, 2)
    want_a, _ = dev.build_lut(a.vectors[0], *a.dqs)
    want_b, shape_b = dev.build_lut(b.vectors[0], *b.dqs)
    assert not np.array_equal(want_a, want_b)
    assert dev.device_logtab() is not None
    _clear_status(dev)
    lut_a, _ = dev.solve_lut(_upload(dev, a), reuse=True)
    assert np.array_equal(lut_a.cpu().numpy(), want_a)
    lut_b, got_shape = dev.solve_lut(_upload(dev, b), reuse=True)
    assert lut_b.data_ptr() == lut_a.data_ptr()
    assert np.array_equal(lut_b.cpu().numpy(), want_b) and got_shape == shape_b
