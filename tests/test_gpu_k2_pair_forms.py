"""
GPU tests (-m gpu) of `k2t_apply_pair<KJ>` (csrc/kbbq_k2_tile.h): the short-lived K2 on 4-bit mate-pair rows of exactly 19
or 13 chunks with the rows' geometry compiled in -- 32-bit chunk arithmetic from the wave's first chunk, the XCDs' eighths
by shifts, the LUT addresses by byte-select instructions.  The launch keeps no switch between the forms, so every case
is compared with the CPU oracle and with the persistent kernel on the same reads, exactly.

Shapes: pairs of 2 x 150 bp (19 chunks per row) and 2 x 100 bp (13), and 2 x 50 bp (7 chunks: still `k2t_apply<true>`);
1, 215, 216, 431, 432 rows -- a workgroup takes 4096 chunks, 215.6 rows of 19 chunks -- and 2000 rows (9.3 workgroups of
19-chunk rows: the eighths the XCDs walk and the remainder that keeps its order both occur); one read group, and 8 read
groups on grouped rows (uneven, one empty) stored in grouped order and through the permutation.
Data: every quality byte 0 .. Qt + 32 occurs inside reads (all rows of the LUT are indexed, bytes 1 .. 32 included), N
bases at random, as a mate's last base and on both sides of every 256th chunk (a wave's first chunk and the base before it).
Expected: the CPU oracle's apply on the same reads, and the persistent kernel (k2v3_apply) on the same reads as character
rows -- the comparison bench.py's `verify` makes.  Both are computed once per read length and only read afterwards.
That model is solved from reads without errors: its LUT is one constant per read group, blind to the cycle, context and
quality-row addresses.  So every (S, R) case is run again under three probe models of tests/k2_probe.py -- all cycle entries
negative against large contexts, and two whose output byte names the column -- against k2_probe.reference_apply.
"""
import os

import numpy as np
import pytest

import k2_probe
from conftest import GOLDEN_CASES, load_golden
from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROWS = 2000
QT = 43                                              # quality rows of the model: bytes 33 .. 75 are served, 76 is not
GROUPS = 8
PROBES = ('negcycle', 'col161', 'col157')
# read group of pair row i on the 8-group cases: uneven shares, group 5 empty
GROUP_OF = np.array([0, 1, 1, 2, 2, 2, 3, 4, 4, 6, 6, 6, 6, 7, 0, 3, 3, 3, 3, 3, 3, 3, 3], dtype=np.uint32)


def _reads(oracle, S, R):
    """2 * ROWS reads of S bases as host planes: synthetic, then the quality bytes and N bases the module's docstring lists."""
    n = 2 * ROWS
    seq, _, qual, meta = oracle.synth(0, n, n, 1000 + S + R, S, S, 1, 0, 41)
    seq, qual, meta = seq.copy(), qual.copy(), meta.copy()
    rng = np.random.default_rng(S + R)
    if R > 1:
        rg = GROUP_OF[np.arange(ROWS) % len(GROUP_OF)]
        meta = (meta & np.uint32(0x8000FFFF)) | (np.repeat(rg, 2) << np.uint32(16))
    # every byte 0 .. 75 as a quality: in the mates of row 0 (the 1-row case) and of every 37th row (all groups: 37 and
    # len(GROUP_OF) have no common factor)
    ramp = np.arange(QT + 33, dtype=np.uint8)
    lo, hi = ramp[:38], ramp[38:]
    for r in range(0, n, 2 * 37):
        qual[r, 3:41] = lo
        qual[r + 1, 5:43] = hi[::-1]
    qual[0, :38] = hi
    qual[1, :38] = lo[::-1]
    assert np.array_equal(np.unique(np.concatenate([qual[0, :S], qual[1, :S]])), ramp)
    # N bases: 2 % at random, the last base of some mates, both sides of every 256th chunk of the pair rows
    seq[:, :S][rng.random((n, S)) < 0.02] = ord('N')
    seq[0:n:11, S - 1] = ord('N')
    seq[1:n:13, S - 1] = ord('N')
    ppitch = (2 * S + 1 + 15) // 16 * 16
    for c in range(256, ROWS * (ppitch // 16), 256):
        for byte in (16 * c - 1, 16 * c):
            row, p = divmod(byte, ppitch)
            if p < S:
                seq[2 * row, p] = ord('N')
            elif S < p <= 2 * S:
                seq[2 * row + 1, p - S - 1] = ord('N')
    return seq, qual, meta


class Case:
    pass


@pytest.fixture(scope='module')
def cases(dev, oracle):
    """Per (S, R): the reads, the LUT of the oracle's model for them, the oracle's new qualities and the persistent
    kernel's on character rows.  Built on first use, read-only afterwards."""
    made = {}

    def get(S, R):
        if (S, R) in made:
            return made[S, R]
        c = Case()
        c.S, c.R = S, R
        c.seq, c.qual, c.meta = _reads(oracle, S, R)
        tabs = oracle.accumulate(c.seq, c.seq, c.qual, c.meta, R, S, minscore=6)
        dqs = oracle.get_delta_qs(*tabs)
        c.model = (tabs[0],) + tuple(dqs)
        lut, c.shape = dev.build_lut(*c.model)
        assert c.shape[3] == dev.N.APPLY_FAST
        c.lut = dev.lut_to_device(lut)
        c.want = oracle.apply(c.seq, c.qual, c.meta, *c.model)[:, :S] + 33            # the oracle returns raw qualities
        assert c.want.min() >= 0 and c.want.max() <= 255
        # the persistent kernel on the same reads as character rows (grouped by read group when there are several)
        b = dev.ReadBatch.from_host(c.seq, c.qual, c.meta, cseq=c.seq)
        saved = {k: os.environ.get(k) for k in ('KBBQ_K2_TILE', 'KBBQ_K2_TILE_CHARS')}
        os.environ.update(KBBQ_K2_TILE='0', KBBQ_K2_TILE_CHARS='0')
        try:
            if R > 1:
                g = dev.group_by_rg(b, R)
                out = dev.ungroup(g, dev.apply(g, c.lut, c.shape))
            else:
                out = dev.apply(b, c.lut, c.shape)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        c.persistent = out[:b.n, :S].cpu().numpy()
        assert np.array_equal(c.persistent, c.want)
        assert (c.want != c.qual[:, :S]).any()
        # the probe models: LUTs that do vary with the cycle and the context, and the reference's bytes under them
        c.probes = {}
        models = [k2_probe.probe(name, R, 2 * S) for name in PROBES]
        # ... which these expectations must keep doing: every probe varies with the cycle, and (the column probes' contexts
        # are 0 by construction) one of them with the cycle and the 16 dinucleotides at once
        assert all(np.ptp(m[3]) > 0 for m in models)
        assert any(np.ptp(m[3]) > 0 and np.ptp(m[4][..., :16]) > 0 for m in models)
        for name, model in zip(PROBES, models):
            lut, shape = dev.build_lut(*model)
            assert shape == c.shape
            want = k2_probe.reference_apply(c.seq, c.qual, c.meta, *model)
            assert want.min() >= 0 and want.max() <= 255 and not want[:, S:].any()
            c.probes[name] = (dev.lut_to_device(lut), want[:, :S].astype(np.uint8))
        made[S, R] = c
        return c
    return get


def _laid(dev, c, rows):
    n = 2 * rows
    b = dev.ReadBatch.from_host(c.seq[:n], c.qual[:n], c.meta[:n], cseq=c.seq[:n])
    laid = dev.lay_out(b, c.R, c.S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch) and not laid.twins and laid.n == rows
    assert laid.pitch // 16 == {150: 19, 100: 13, 50: 7}[c.S]
    assert (laid.seg is not None) == (c.R > 1)
    return b, laid


def _check(c, got, n):
    got = got[:n].cpu().numpy()
    S = c.S
    assert np.array_equal(got[:, :S], c.want[:n])
    assert np.array_equal(got[:, :S], c.persistent[:n])
    assert not got[:, S:].any()


def _check_probes(dev, c, b, laid, n, **how):
    """The same rows under every probe LUT against the reference's bytes."""
    for name in PROBES:
        lut, want = c.probes[name]
        out = dev.apply(laid, lut, c.shape, **how)
        if laid.seg is not None and not how.get('restore_order'):
            out = dev.ungroup(laid, out)
        got = laid.unpack(out, b.pitch)[:n].cpu().numpy()
        assert np.array_equal(got[:, :c.S], want[:n]), name
        assert not got[:, c.S:].any(), name


@pytest.mark.parametrize('rows', [1, 215, 216, 431, 432, ROWS])
@pytest.mark.parametrize('S', [150, 100, 50])
def test_one_read_group(dev, cases, S, rows):
    c = cases(S, 1)
    b, laid = _laid(dev, c, rows)
    out = dev.apply(laid, c.lut, c.shape)
    plane = out[:rows].cpu().numpy()
    assert not plane[:, S].any() and not plane[:, 2 * S + 1:].any()          # separator and padding stay 0
    _check(c, laid.unpack(out, b.pitch), 2 * rows)
    _check_probes(dev, c, b, laid, 2 * rows)


@pytest.mark.parametrize('restore', [False, True])
@pytest.mark.parametrize('S', [150, 100, 50])
def test_eight_read_groups_on_grouped_rows(dev, cases, S, restore):
    c = cases(S, GROUPS)
    b, laid = _laid(dev, c, ROWS)
    sizes = np.diff(laid.seg.cpu().numpy())
    assert sizes[5] == 0 and len(set(sizes.tolist())) >= 5 and sizes.sum() == ROWS
    out = dev.apply(laid, c.lut, c.shape, restore_order=restore)
    if not restore:
        out = dev.ungroup(laid, out)
    _check(c, laid.unpack(out, b.pitch), 2 * ROWS)
    _check_probes(dev, c, b, laid, 2 * ROWS, restore_order=restore)


@pytest.mark.parametrize('what', ['quality', 'nibble', 'read_group'])
@pytest.mark.parametrize('S', [150, 100])
def test_what_the_kernel_cannot_serve_is_reported_as_before(dev, oracle, cases, S, what):
    """One chunk the table-driven kernel cannot serve: the launch ends with the LUT status (LutNeedsCheckedApply), as the
    kernel before this change reports it; on character rows `apply` then re-runs the checked kernel, which decides as the
    oracle does (IndexError for a quality of 43 and for a read group the model does not have)."""
    c = cases(S, 1)
    rows, row = 432, 217                              # the second workgroup of 19-chunk rows
    b, laid = _laid(dev, c, rows)
    seq, qual, meta = c.seq[:2 * rows].copy(), c.qual[:2 * rows].copy(), c.meta[:2 * rows].copy()
    if what == 'quality':
        laid.qual[row, S + 1 + 40] = QT + 33          # mate 2, base 40
        qual[2 * row + 1, 40] = QT + 33
    elif what == 'nibble':
        laid.seq[row, 19] = (int(laid.seq[row, 19]) & 0x0F) | 0x60
    else:
        laid.meta[row] = int(laid.meta[row]) | (1 << 16)
        meta[2 * row:2 * row + 2] |= np.uint32(1 << 16)
    with pytest.raises(dev.N.LutNeedsCheckedApply):
        dev.apply(laid, c.lut, c.shape)
    if what != 'nibble':                              # (a nibble that is no code has no character row)
        with pytest.raises(IndexError):
            oracle.apply(seq, qual, meta, *c.model)
        with pytest.raises(IndexError):
            dev.apply(dev.ReadBatch.from_host(seq, qual, meta, cseq=seq), c.lut, c.shape)
    # the batch as it was is served again
    _, laid = _laid(dev, c, rows)
    _check(c, laid.unpack(dev.apply(laid, c.lut, c.shape), b.pitch), 2 * rows)


def test_one_read_per_row_under_a_narrowed_lut(dev, oracle):
    """Reads of 36 .. 100 bases, one to a row on 4-bit planes (`k2t_apply<true>` under the LUT narrowed to the rows' pitch,
    k3_fill_row_lut, which cannot be read from outside the library): every quality byte 0 .. 75 occurs, second-in-pair
    reads (the mirrored cycle entries) included."""
    n, S = 3000, 100
    seq, _, qual, meta = oracle.synth(0, n, n, 77, 36, S, 1, 0, 41)
    seq, qual, meta = seq.copy(), qual.copy(), meta.copy()
    lens = (meta & 0xFFFF).astype(np.int64)
    ramp = np.arange(QT + 33, dtype=np.uint8)
    for r in range(0, n, 29):
        L = int(lens[r])
        qual[r, :min(L, 38)] = ramp[:min(L, 38)] if r % 2 else ramp[38:38 + min(L, 38)]
    assert np.array_equal(np.unique(np.concatenate([qual[r, :lens[r]] for r in range(0, n, 29)])), ramp)
    tabs = oracle.accumulate(seq, seq, qual, meta, 1, S, minscore=6)
    model = (tabs[0],) + tuple(oracle.get_delta_qs(*tabs))
    want = oracle.apply(seq, qual, meta, *model) + 33
    lut, shape = dev.build_lut(*model)
    b = dev.ReadBatch.from_host(seq, qual, meta, cseq=seq)
    laid = dev.lay_out(b, 1, S, packed=True)
    assert laid.nib and isinstance(laid, dev.ReadBatch) and laid.pitch == 112 and 2 * S > laid.pitch
    got = dev.apply(laid, dev.lut_to_device(lut), shape)[:n].cpu().numpy()
    for r in range(n):
        assert np.array_equal(got[r, :lens[r]], want[r, :lens[r]]), r
        assert not got[r, lens[r]:].any()


@pytest.mark.parametrize('minscore', [6, 0, 20])
@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_rows_below_the_threshold_are_the_analytic_form(dev, name, minscore):
    """What the LUT builders give a quality byte below 33 + minscore, on the LUT bytes themselves: row r of a read group
    holds (int8)(r - 33) over its cycle entries and 0 behind them (contexts and slack) -- in the pair LUT (mate-pair rows
    and rows of two first-in-pair reads) and in the blob's own full LUT, the form k3_fill_row_lut narrows.  A kernel
    that writes these rows in the LDS instead of staging them (profiles/r08_k2_pair_forms.md: measured, not kept) may
    rely on exactly this."""
    import torch
    from kbbq import _native as N
    _, g = load_golden(name)
    blob, shape = dev.build_lut(g['meanq'], g['rgdq'], g['qdq'], g['posdq'], g['dinucdq'], minscore=minscore)
    R, Qt, S2 = shape[:3]
    assert Qt == QT
    lib = N.load()
    n_const = 33 + min(minscore, Qt)

    def check(rows, ctx_off):
        rows = rows.view(np.int8).reshape(R, 33 + Qt, -1)
        rb = rows.shape[2]
        assert rb % 4 == 0 and (rb // 4) % 2 == 1 and ctx_off % 4 == 0 and ctx_off + 25 <= rb
        want = np.zeros((n_const, rb), dtype=np.int8)
        want[:, :ctx_off] = (np.arange(n_const) - 33)[:, None]
        for r in range(R):
            assert np.array_equal(rows[r, :n_const], want), (name, r)
        assert rows[:, n_const:].any() or n_const == 33 + Qt

    # the blob's full LUT: [0, W) forward, [W, 2 W) mirrored, contexts at 2 W, W = S2 + 16
    off = (R * Qt * lib.kbbq_lut_row_stride(S2) * 2 + 15) & ~15
    check(np.frombuffer(blob, dtype=np.uint8)[off:off + lib.kbbq_full_lut_bytes(R, Qt, S2)], 2 * (S2 + 16))
    # the pair LUT: contexts behind the row's pitch
    d_lut = dev.lut_to_device(blob)
    ctx = dev.context(d_lut.device.index)
    nbytes = lib.kbbq_pair_lut_bytes(R, Qt, S2)
    for flags in (N.ROWS_PAIRS | N.ROWS_NIBBLES, N.ROWS_PAIRS | N.ROWS_NIBBLES | N.ROWS_TWINS):
        plut = torch.empty(nbytes, dtype=torch.uint8, device=d_lut.device)
        N.check(lib.kbbq_pair_lut_rows_dev(ctx.handle, N.ptr(d_lut), R, S2, minscore, flags, N.ptr(plut)))
        ctx.sync()
        check(plut.cpu().numpy(), lib.kbbq_pair_pitch(S2))
