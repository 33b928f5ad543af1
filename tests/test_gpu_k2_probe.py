"""
GPU tests (-m gpu) of every form of K2 (the apply kernels) under the probe models of tests/k2_probe.py: LUTs whose output
byte names the looked-up column, context, quality row and read group, with entries on both int8 ends and sums of exactly
0 and 255.  Every case uploads a probe's blob (`dev.build_lut` + `dev.lut_to_device`), runs `dev.apply` /
`dev.apply_bands` and compares ALL bytes of the plane with `k2_probe.reference_apply` (a NumPy gather that knows
neither the oracle nor the product); bytes at and beyond a read's end are 0 there, so they must be 0 here.

Which kernel a case reaches (csrc/kbbq_hip.hip: kbbq_apply_dev, apply_rows, k2_tile_serves, launch_k2v3,
kbbq_apply_bands_dev; the switches are the ones the launch layer reads):

  character rows, one read group (test_character_rows_of_one_read_group) -- kbbq_apply_dev in fast mode with R = 1 goes to
      apply_rows when k2_tile_serves: a read group's LUT, narrowed to Sb = min(pitch, S2) columns (k3_fill_row_lut), is at most
      52 KB.  150 and 151 bases in pitch 160 under 300 / 302 columns (29 KB) and 40 bases in pitch 48 under 600 columns
      (Sb = 48, 12 KB): `k2t_apply<false>`.  KBBQ_K2_TILE_CHARS=0: k2_tile_serves declines, the LUT fits the LDS:
      `k2v3_apply<false>` on the same narrowed LUT.  KBBQ_K2_ROWLUT=0: Sb = S2, the blob's own full LUT as
      fill_full_lut_host wrote it -- 51 KB at 300 columns, still `k2t_apply<false>`; 96 KB at 600, `k2v3_apply<false>`.
  character rows, 3 read groups, not grouped (test_character_rows_of_several_read_groups[3]) -- R != 1 and no segments:
      k2_tile_serves declines; 3 x 76 rows of the LUT narrowed to pitch 112 are 67 KB: `k2v3_apply<false>` with every group's
      rows in the LDS.
  character rows, 8 read groups, 300 columns, not grouped ([8]) -- 8 x 76 x 388 B = 236 KB do not fit the LDS; the one-byte
      copy of the canonical LUT (8 x 43 x 326 B = 112 KB) does: `k2_apply<int8_t, true, false>`.
  the same rows in mode APPLY_CHECKED (test_checked_mode) -- kbbq_apply_dev skips both fast branches: the int16 LUT staged,
      `k2_apply<int16_t, true, true>`, for 1 and 3 read groups (28 KB, 60 KB); 8 groups x 300 columns are 224 KB of int16:
      `k2_apply<int16_t, false, true>` reads the LUT from global memory.
  4-bit planes, one read per row (test_four_bit_rows) -- apply_rows with nib = 1; one read group, or rows grouped by read
      group (k2_tile_serves takes grouped rows): `k2t_apply<true>`, on grouped rows behind `k2t_plan` and, stored through
      `perm` (restore_order), `k2t_order`.  KBBQ_K2_TILE=0: `k2v3_apply<true>`, one grid slice per group.
  4-bit mate-pair rows (test_mate_pair_rows) -- the pair LUT of k3_fill_pair_lut; 2 x 150 and 2 x 100 bp are 19 and 13
      chunks: k2t_pair_form picks `k2t_apply_pair<19>` / `<13>`, on planes with the error bit (lay_out's default when the
      batch has corrected reads) the `<.., true>` instances; 2 x 50 bp are 7 chunks: `k2t_apply<true>` on the pair LUT.
      KBBQ_K2_TILE=0: `k2v3_apply<true>` / `<true, true>`.
  single-end reads two to a row (test_twins_rows) -- the same kernels under the twins form of the pair LUT (a row's second
      half reads the forward columns).
  mixed lengths 36 .. 300, one read group (test_all_length_bands_in_one_launch) -- kbbq_apply_bands_dev merges the eight
      4-bit bands into `k2t_bands`, every band under the LUT narrowed to its pitch (51 KB at pitch 304).

Rows: a short-lived workgroup takes 4096 chunks and the walk of the XCDs' eighths starts at 8 workgroups, so the tile routes run
on 1 row and on the fewest rows that give 9 workgroups (8 remapped, one that keeps its place) -- on grouped rows, 9 workgroups
for the group that owns 12 rows of 20.  The persistent and checked routes take 1 row and about 2000.
Reads and references are built once per shape (module fixture) and only read afterwards.
"""
import numpy as np
import pytest

import k2_probe as P
from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

WG_CHUNKS = 4096


def rows_for(cpr, share=1.0):
    """The fewest rows of `cpr` chunks with 9 workgroups (for the group that owns `share` of them), rounded up to 10."""
    return (int(np.ceil((8 * WG_CHUNKS + 1) / cpr / share)) + 9) // 10 * 10


class Shape:
    pass


# key -> (S, R, pitch, S2, reads, keywords of k2_probe.reads)
SHAPES = {
    'c150': (150, 1, 160, 300, rows_for(10), dict(len_lo=50)),
    'c151': (151, 1, 160, 302, rows_for(10), dict(len_lo=50)),
    'c40': (40, 1, 48, 600, rows_for(3), dict(len_lo=14)),
    'c100x3': (100, 3, 112, 200, 2000, dict(len_lo=34)),
    'c150x8': (150, 8, 160, 300, 2000, dict(len_lo=50)),
    'n150x8': (150, 8, 160, 300, rows_for(10, 0.6), dict(len_lo=50)),
    'p150': (150, 1, 160, 300, 2 * rows_for(19), {}),
    'p150x8': (150, 8, 160, 300, 2 * rows_for(19, 0.6), {}),
    'p100': (100, 1, 112, 200, 2 * rows_for(13), {}),
    'p100x8': (100, 8, 112, 200, 2 * rows_for(13, 0.6), {}),
    'p50': (50, 1, 64, 100, 2 * rows_for(7), {}),
    'p50x8': (50, 8, 64, 100, 2 * rows_for(7, 0.6), {}),
    't100': (100, 1, 112, 200, 2 * rows_for(13), dict(single_end=True)),
    't50x3': (50, 3, 64, 100, 2 * rows_for(7, 0.6), dict(single_end=True)),
}
BANDS = [(36, 48), (49, 64), (65, 96), (97, 128), (129, 160), (161, 208), (209, 256), (257, 300)]
for _lo, _hi in BANDS:
    _pitch = (_hi + 15) // 16 * 16
    SHAPES['b%d' % _hi] = (_hi, 1, _pitch, 600, rows_for(_pitch // 16), dict(len_lo=_lo))


@pytest.fixture(scope='module')
def shapes():
    made = {}

    def get(key):
        if key not in made:
            s = Shape()
            s.S, s.R, s.pitch, s.S2, s.n, kw = SHAPES[key]
            s.n += s.n % 2
            s.seq, s.cseq, s.qual, s.meta = P.reads(s.S, s.R, s.n, seed=sum(key.encode()), pitch=s.pitch, S2=s.S2, **kw)
            s.want, s.look = {}, P.lookups(s.seq, s.qual, s.meta, s.S2)
            made[key] = s
        return made[key]
    return get


def want_of(s, name):
    """The reference's bytes for shape `s` under probe `name` (uint8 [n, pitch]), computed once."""
    if name not in s.want:
        w = P.reference_apply(s.seq, s.qual, s.meta, *P.probe(name, s.R, s.S2))
        assert w.min() >= 0 and w.max() <= 255
        s.want[name] = w.astype(np.uint8)
        s.want[name].setflags(write=False)
    return s.want[name]


@pytest.fixture(scope='module')
def luts(dev):
    made = {}

    def get(name, R, S2):
        if (name, R, S2) not in made:
            blob, shape = dev.build_lut(*P.probe(name, R, S2))
            assert shape == (R, P.QT, S2, dev.N.APPLY_FAST), name
            made[name, R, S2] = (dev.lut_to_device(blob), shape)
        return made[name, R, S2]
    return get


def _batch(dev, s, n):
    return dev.ReadBatch.from_host(s.seq[:n], s.qual[:n], s.meta[:n], cseq=s.cseq[:n])


def _compare(s, name, got, n):
    got = got[:n].cpu().numpy()
    want = want_of(s, name)[:n]
    if got.shape[1] != want.shape[1]:                                   # (a plane unpacked at another pitch)
        assert not got[:, s.S:].any()
        got, want = got[:, :s.S], want[:, :s.S]
    bad = np.argwhere(got != want)
    assert not len(bad), '%s: %d bytes differ, the first at read %d, base %d: %d, not %d' % (
        name, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def _every_probe(dev, s, luts, n, run):
    for name in P.PROBES:
        lut, shape = luts(name, s.R, s.S2)
        _compare(s, name, run(lut, shape), n)
    # the ends of the contract are in these very rows, on counted bases
    if n > 1000:
        w = want_of(s, 'context')[:n]
        counted = s.look.counted[:n]
        assert (w[counted] == 0).any() and (w[counted] == 255).any()


ROWS = ['one row', 'many rows']


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('switch', ['tile', 'KBBQ_K2_TILE_CHARS', 'KBBQ_K2_ROWLUT'])
@pytest.mark.parametrize('key', ['c150', 'c151', 'c40'])
def test_character_rows_of_one_read_group(dev, shapes, luts, monkeypatch, key, switch, rows):
    s = shapes(key)
    if switch != 'tile':
        monkeypatch.setenv(switch, '0')
    n = 1 if rows == 'one row' else s.n
    b = _batch(dev, s, n)
    _every_probe(dev, s, luts, n, lambda lut, shape: dev.apply(b, lut, shape))


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('key', ['c100x3', 'c150x8'])
def test_character_rows_of_several_read_groups(dev, shapes, luts, key, rows):
    s = shapes(key)
    n = 1 if rows == 'one row' else s.n
    b = _batch(dev, s, n)
    _every_probe(dev, s, luts, n, lambda lut, shape: dev.apply(b, lut, shape))


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('key', ['c150', 'c40', 'c100x3', 'c150x8'])
def test_checked_mode(dev, shapes, luts, key, rows):
    s = shapes(key)
    n = 1 if rows == 'one row' else min(s.n, 2000)
    b = _batch(dev, s, n)
    _every_probe(dev, s, luts, n, lambda lut, shape: dev.apply(b, lut, shape[:3] + (dev.N.APPLY_CHECKED,)))


def _ordered(dev, laid, out, restore):
    return out if (restore or laid.seg is None) else dev.ungroup(laid, out)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('switch', ['tile', 'KBBQ_K2_TILE'])
@pytest.mark.parametrize('key,restore', [('c150', False), ('n150x8', False), ('n150x8', True)])
def test_four_bit_rows(dev, shapes, luts, monkeypatch, key, restore, switch, rows):
    s = shapes(key)
    if switch != 'tile':
        monkeypatch.setenv(switch, '0')
    n = 1 if rows == 'one row' else s.n
    laid = dev.lay_out(_batch(dev, s, n), s.R, s.S, packed=True, pairs=False)
    assert laid.nib and isinstance(laid, dev.ReadBatch) and laid.pitch == s.pitch and (laid.seg is not None) == (s.R > 1)
    if s.R > 1 and n > 1:
        sizes = np.diff(laid.seg.cpu().numpy())
        assert sizes[5] == 0 and sizes[3] * (s.pitch // 16) > 8 * WG_CHUNKS
    _every_probe(dev, s, luts, n, lambda lut, shape: _ordered(dev, laid, dev.apply(laid, lut, shape, restore_order=restore), restore))


# (shape, stored through perm, planes with the error bit): rows of 7 chunks carry no error bit
PAIR_CASES = [(key, restore, errbit) for errbit in (False, True)
              for key, restore in (('p150', False), ('p150x8', False), ('p150x8', True), ('p100', False), ('p100x8', False), ('p100x8', True))]
PAIR_CASES += [('p50', False, False), ('p50x8', True, False)]


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('switch', ['tile', 'KBBQ_K2_TILE'])
@pytest.mark.parametrize('key,restore,errbit', PAIR_CASES)
def test_mate_pair_rows(dev, shapes, luts, monkeypatch, key, restore, errbit, switch, rows):
    s = shapes(key)
    if switch != 'tile':
        monkeypatch.setenv(switch, '0')
    n = 2 if rows == 'one row' else s.n
    b = _batch(dev, s, n)
    laid = dev.lay_out(b, s.R, s.S, packed=True, errbit=errbit)
    assert laid.nib and isinstance(laid, dev.PairBatch) and not laid.twins and laid.errbit == errbit and laid.n == n // 2
    assert laid.pitch // 16 == {150: 19, 100: 13, 50: 7}[s.S] and (laid.seg is not None) == (s.R > 1)
    if errbit:
        assert (s.seq[:n] != s.cseq[:n]).any()                       # bit 3 is set in some nibbles
    if s.R > 1 and n > 2:
        assert np.diff(laid.seg.cpu().numpy())[3] * (laid.pitch // 16) > 8 * WG_CHUNKS
    _every_probe(dev, s, luts, n, lambda lut, shape: laid.unpack(
        _ordered(dev, laid, dev.apply(laid, lut, shape, restore_order=restore), restore), b.pitch))


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('switch', ['tile', 'KBBQ_K2_TILE'])
@pytest.mark.parametrize('key', ['t100', 't50x3'])
def test_twins_rows(dev, shapes, luts, monkeypatch, key, switch, rows):
    s = shapes(key)
    if switch != 'tile':
        monkeypatch.setenv(switch, '0')
    n = 2 if rows == 'one row' else s.n
    b = _batch(dev, s, n)
    laid = dev.lay_out(b, s.R, s.S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch) and laid.twins and laid.n == n // 2
    _every_probe(dev, s, luts, n, lambda lut, shape: laid.unpack(dev.apply(laid, lut, shape, restore_order=True), b.pitch))


def test_all_length_bands_in_one_launch(dev, shapes, luts):
    bands = [shapes('b%d' % hi) for _, hi in BANDS]
    items = []
    for (lo, hi), s in zip(BANDS, bands):
        laid = dev.lay_out(_batch(dev, s, s.n), 1, s.S, packed=True, pairs=False)
        assert laid.nib and isinstance(laid, dev.ReadBatch) and laid.pitch == s.pitch and laid.seg is None
        items.append((laid, hi, lo))
    ctx = dev.context()
    for name in P.PROBES:
        lut, shape = luts(name, 1, 600)
        ctx.kernel_ms(1, reset=True); ctx.timing(True)
        outs = dev.apply_bands(items, lut, shape)
        ctx.timing(False)
        assert ctx.kernel_ms(1)[1] == 1                                  # one launch: k2t_bands took every band
        for s, out in zip(bands, outs):
            _compare(s, name, out, s.n)


# ---------------------------------------------------------------------------------------------------- the ends of the contract
def _held_late(s, ctx):
    """A (r, q, col) that a counted base of context `ctx` looks up, chosen so that the lowest read holding it comes as late as
    possible; returns (r, q, col, that read)."""
    L = s.look
    m = L.ctx == ctx
    key = (L.r[m] * P.QT + L.q[m]) * s.S2 + L.col[m]
    order = np.lexsort((L.row[m], key))
    key, row = key[order], L.row[m][order]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    k = int(np.argmax(row[first]))
    cell, read = int(key[first][k]), int(row[first][k])
    return cell // (P.QT * s.S2), cell // s.S2 % P.QT, cell % s.S2, read


@pytest.mark.parametrize('end', ['low', 'high'])
@pytest.mark.parametrize('key', ['c150', 'c100x3', 'c150x8'])
def test_one_past_the_range_is_a_range_error_at_the_first_read_that_leaves_it(dev, shapes, key, end):
    """Checked routes: the context probe with one cycle cell moved by one, so that exactly the bases that look up that cell
    with context AA (no context) sum to -1 (256).  The blob says "not range-safe"; `apply` runs the checked kernel, which
    reports KBBQ_E_RANGE (ValueError) at the lowest such read -- and serves the rows in front of it, where nobody holds
    the combination, with the reference's bytes and no error."""
    s = shapes(key)
    r, q, col, read = _held_late(s, P.ONE_PAST_CTX[end])
    assert read > 0
    model = (P.one_past_low if end == 'low' else P.one_past_high)(s.R, s.S2, r, q, col)
    assert P.fast_range(model) == 2
    blob, shape = dev.build_lut(*model)
    assert shape[3] == dev.N.APPLY_CHECKED
    lut = dev.lut_to_device(blob)
    n = min(s.n, read + 200)
    want = P.reference_apply(s.seq[:n], s.qual[:n], s.meta[:n], *model)
    out_of_range = np.nonzero(((want < 0) | (want > 255)).any(axis=1))[0]
    assert out_of_range[0] == read and want[read].min() >= -1 and want[read].max() <= 256
    with pytest.raises(ValueError) as err:
        dev.apply(_batch(dev, s, n), lut, shape)
    assert err.value.read_index == read
    got = dev.apply(_batch(dev, s, read), lut, shape)[:read].cpu().numpy()
    assert np.array_equal(got, want[:read])
    # the layouts of the fast kernels have no checked form: they say so before anything is launched
    laid = dev.lay_out(_batch(dev, s, read + (read & 1)), s.R, s.S, packed=True, pairs=False)
    with pytest.raises(dev.N.LutNeedsCheckedApply):
        dev.apply(laid, lut, shape)


@pytest.mark.parametrize('key', ['c150', 'c100x3', 'c150x8'])
def test_entries_beyond_int8_are_served_by_the_checked_kernels(dev, shapes, key):
    s = shapes(key)
    model = P.int8_misfit(s.R, s.S2)
    blob, shape = dev.build_lut(*model)
    assert shape[3] == dev.N.APPLY_CHECKED and P.fast_range(model) == 1
    n = min(s.n, 2000)
    want = P.reference_apply(s.seq[:n], s.qual[:n], s.meta[:n], *model)
    assert (want[s.look.counted[:n]] == 133).all()
    got = dev.apply(_batch(dev, s, n), dev.lut_to_device(blob), shape)[:n].cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize('key', ['p150', 'p100x8', 'p50', 'c150', 't100'])
def test_the_layouts_refuse_checked_mode(dev, shapes, luts, key):
    """4-bit and mate-pair layouts in mode APPLY_CHECKED: LutNeedsCheckedApply, as `_device.apply` documents."""
    s = shapes(key)
    laid = dev.lay_out(_batch(dev, s, 64), s.R, s.S, packed=True, pairs=None if key[0] in 'pt' else False)
    assert laid.nib
    lut, shape = luts('context', s.R, s.S2)
    with pytest.raises(dev.N.LutNeedsCheckedApply):
        dev.apply(laid, lut, shape[:3] + (dev.N.APPLY_CHECKED,))


def test_a_quality_beyond_the_model_is_the_references_index_error(dev, shapes, luts):
    """Byte 76 (quality 43) has no model row: the reference raises IndexError, and so do the character rows (the tile kernel
    reports the chunk, `apply` re-runs the checked kernel, which decides)."""
    s = shapes('c150')
    n = 500
    qual = s.qual[:n].copy()
    qual[321, 7] = 33 + P.QT
    model = P.probe('context', 1, s.S2)
    with pytest.raises(IndexError):
        P.reference_apply(s.seq[:n], qual, s.meta[:n], *model)
    lut, shape = luts('context', 1, s.S2)
    with pytest.raises(IndexError) as err:
        dev.apply(dev.ReadBatch.from_host(s.seq[:n], qual, s.meta[:n]), lut, shape)
    assert err.value.read_index == 321
