"""
GPU tests (-m gpu) of the aligned ApplyBQSR kernel (kaa_apply, csrc/kbbq_apply_aligned.h) under the probe models and rows of
tests/aligned_apply_probe.py.  Every case calls kbbq_apply_aligned_dev on device planes, into an output plane prefilled with
0xEE, and compares ALL its bytes with `reference_apply` (NumPy; knows neither the oracle nor the product); the model blobs come
from applybqsr._model, which must choose the form the probe is meant for; `kbbq_ctx_status` is read after every call.

Which shape reaches what (aligned_apply_probe.SHAPES; test_aligned_apply_probe_host.py asserts that the rows do reach it):
  p16     257 x 16    L 0..16, full rows beside L = 0 rows; 257 chunks: a full workgroup, then one with ONE live lane and 255
                      lanes clamped onto it
  p48     200 x 48    L on both sides of every chunk edge; 3 chunks a row: rows straddle wave and workgroup edges at every phase
  p160    103 x 160   L 150 / 151 / 160 under 300 / 302 / 320 columns: every column by the mate that reaches it
  p1040   9 x 1040    65 chunks a row: every wave's lane 0 and lane 63 sit mid-row (the neighbour bytes that come from memory)
  long    3 x 65536   L 65535 / 65521 / 4097 under 65536 columns: columns beyond 32767, read 2 mirrored from the far end, F64
                      rows of 65554 doubles, all 17 contexts at both ends of a wave on both strands
  rg4096  64 x 32     read groups 0, 1, 2047, 2048, 4095 of 4096; bases at j >= S2 below minscore raise nothing
  qt95    64 x 48     LUT with 95 quality rows (bytes up to 127), minscore 0 / 2 / 20 beside the context's fixed 6
  qt223   64 x 48     F64 with 223 quality rows (bytes up to 255)
No case hands the kernel a row outside the header's preconditions (rg >= R, L > pitch, unaligned or missing planes); those
reach only the argument checks, which launch nothing.
"""
import ctypes

import numpy as np
import pytest

import aligned_apply_probe as P
from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


class Kernel:
    """kbbq_apply_aligned_dev / _q_dev on host planes: uploads, runs, returns (output plane, status code, row)."""

    def __init__(self, dev):
        import torch
        from kbbq import _native as N
        from kbbq.gatk import applybqsr
        self.N, self.T, self.A = N, torch, applybqsr
        self.ctx, self.lib = dev.context(), N.load()
        self.code = {TypeError: N.KBBQ_E_TYPE, IndexError: N.KBBQ_E_INDEX, P.RangeError: N.KBBQ_E_RANGE, None: N.KBBQ_OK}

    def up(self, x):
        if x is None:
            return None
        x = np.ascontiguousarray(x) if x.flags.writeable else np.array(x)
        return self.T.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()

    def blob(self, model, mode, how='_model', minscore=6):
        """(device blob, mode constant, R, Qt, S2): through applybqsr._model, which must choose `mode`, or the float64 rows."""
        N = self.N
        want = N.ALIGNED_LUT if mode == 'lut' else N.ALIGNED_F64
        R, Qt, S2 = np.asarray(model[3]).shape
        if how == 'rows':
            return self.up(P.f64_rows(model).view(np.uint8).reshape(-1)), want, R, Qt, S2
        got, blob, R_, Qt_, S2_ = self.A._model(*model, minscore)
        assert (R_, Qt_, S2_) == (R, Qt, S2)
        if mode is not None:
            assert got == want, 'applybqsr._model chose form %d' % got
        return self.up(blob), got, R, Qt, S2

    def status(self):
        row = ctypes.c_int64(-1)
        return self.lib.kbbq_ctx_status(self.ctx.handle, ctypes.byref(row)), row.value

    def run(self, d, n, pitch, blob, minscore=6, qmap=None):
        """d: device (seq, qual, oq, meta), qual or oq may be None.  -> (plane [n, pitch] uint8, status, row); the status is
        clean afterwards."""
        N = self.N
        d_model, mode, R, Qt, S2 = blob
        d_out = self.T.full((n, pitch), 0xEE, dtype=self.T.uint8, device='cuda')
        args = (self.ctx.handle, N.ptr(d[0]), N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]), n, pitch, R, Qt, S2, minscore, N.ptr(d_model),
                mode, N.ptr(d_out))
        if qmap is None:
            N.check(self.lib.kbbq_apply_aligned_dev(*args))
        else:
            N.check(self.lib.kbbq_apply_aligned_q_dev(*args, N.ptr(qmap)))
        status = self.status()
        assert self.status() == (N.KBBQ_OK, -1)
        return d_out.cpu().numpy(), status[0], status[1]


@pytest.fixture(scope='module')
def kernel(dev):
    return Kernel(dev)


@pytest.fixture(scope='module')
def planes():
    made = {}

    def get(key):
        if key not in made:
            made[key] = P.rows(key, 0)
            for x in made[key]:
                x.setflags(write=False)
        return made[key]
    return get


def _same(got, want, what):
    assert want.min() >= 0 and want.max() <= 255, what
    bad = np.argwhere(got != want)
    assert not len(bad), '%s: %d bytes differ, the first at row %d, byte %d: %d, not %d' % (
        what, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize('key', list(P.SHAPES))
def test_every_model_on_every_shape(kernel, planes, key):
    s = P.SHAPES[key]
    host = planes(key)
    d = [kernel.up(x) for x in host]
    for S2 in s.S2s:
        for name, model, mode, how in P.models(key, S2):
            blob = kernel.blob(model, mode, how)
            for minscore in s.minscores:
                want = P.reference_apply(*host, model, minscore, mode)
                got, status, row = kernel.run(d, s.n, s.pitch, blob, minscore)
                assert (status, row) == (kernel.N.KBBQ_OK, -1), (name, S2, minscore)
                _same(got, want, '%s, %s under %d columns, minscore %d' % (key, name, S2, minscore))
            del blob


# ---------------------------------------------------------------------------------------------------- plane identity
def test_one_plane_and_missing_planes(kernel, planes):
    seq, qual, oq, meta = planes('p48')
    s = P.SHAPES['p48']
    model = P.int_probes(s.R, 96)['col161']
    for mode, how in (('lut', '_model'), ('f64', 'rows')):
        blob = kernel.blob(model, mode, how)
        d_seq, d_qual, d_copy, d_oq, d_meta = (kernel.up(x) for x in (seq, qual, qual.copy(), oq, meta))
        # one plane passed twice, bits 28 / 29 whatever they are: the two-plane call on a copy of it
        want = P.reference_apply(seq, qual, qual, meta, model, 6, mode)
        one = kernel.run((d_seq, d_qual, d_qual, d_meta), s.n, s.pitch, blob)
        two = kernel.run((d_seq, d_qual, d_copy, d_meta), s.n, s.pitch, blob)
        assert one[1:] == two[1:] == (kernel.N.KBBQ_OK, -1)
        _same(one[0], want, 'one plane'), _same(two[0], want, 'a copy')
        # no row selects OQ: d_oq may be missing; no row selects QUAL: d_qual may be
        for bits, d_q, d_o, name in ((0, d_qual, None, 'no OQ'), (3 << 28, None, d_oq, 'no QUAL')):
            m = ((meta & np.uint32(~(3 << 28) & 0xFFFFFFFF)) | np.uint32(bits)).astype(np.uint32)
            want = P.reference_apply(seq, qual, oq, m, model, 6, mode)
            d_m = kernel.up(m)
            both = kernel.run((d_seq, d_qual, d_oq, d_m), s.n, s.pitch, blob)
            missing = kernel.run((d_seq, d_q, d_o, d_m), s.n, s.pitch, blob)
            assert both[1:] == missing[1:] == (kernel.N.KBBQ_OK, -1)
            _same(both[0], want, name + ', both planes given'), _same(missing[0], want, name)


# ---------------------------------------------------------------------------------------------------- statuses
LETTERS = np.frombuffer(b'ACGTTGCA', dtype=np.uint8)
Q, CELL_Q = 30, 31                   # every clean base; the quality that selects a model's special cell


def _clean(n, pitch, L, S2, phase=0):
    """n rows of L bases ACGTTGCA..., source QUAL (30) and context OQ (31) on different planes; bases at j >= S2 have source
    quality 2.  Rows take strand and mate in turn (row k with (k + phase) % 4 == 0 is forward and a first mate); no base is
    an N."""
    i = np.arange(pitch)
    seq = np.where(i < L, LETTERS[i % 8], 0).astype(np.uint8)[None, :].repeat(n, axis=0)
    k = (np.arange(n) + phase) % 4
    rev, second = k & 1, (k >> 1) & 1
    j = np.where(rev[:, None] == 1, L - 1 - i[None, :], i[None, :])
    inside = (i < L)[None, :]
    qual = np.where(inside, np.where(j >= S2, 33 + 2, 33 + Q), 0).astype(np.uint8)
    oq = np.where(inside, 33 + Q + 1, 0).astype(np.uint8).repeat(n, axis=0)
    meta = (L | (1 << 29) | (rev << 30) | (second << 31)).astype(np.uint32)
    return seq, qual, oq, meta


def _i(meta_word, j):
    """The aligned position of sequencing index j in a row."""
    L = int(meta_word) & 0xFFFF
    return L - 1 - j if (int(meta_word) >> 30) & 1 else j


def _forms(kernel, model, minscore=6):
    """The blobs a model runs under: integer models as the LUT of _model and as float64 rows; float models as _model folds them
    (whichever form it proves exact) and as float64 rows."""
    integer = all(np.asarray(x).dtype.kind in 'iu' for x in model)
    return [('lut' if integer else 'f64', kernel.blob(model, 'lut' if integer else None, '_model', minscore)),
            ('f64', kernel.blob(model, 'f64', 'rows'))]


def _expect(kernel, planes_, model, minscore=6, want_error='any'):
    """Runs the batch under every form of the model and expects what the reference says: the bytes, or the code and the row."""
    seq, qual, oq, meta = planes_
    n, pitch = seq.shape
    d = [kernel.up(x) for x in planes_]
    seen = None
    for mode, blob in _forms(kernel, model, minscore):
        X = P.analyse(seq, qual, oq, meta, model, minscore, mode)
        got, status, row = kernel.run(d, n, pitch, blob, minscore)
        if X.error is None:
            assert (status, row) == (kernel.N.KBBQ_OK, -1), mode
            _same(got, X.out, mode)
        else:
            assert (status, row) == (kernel.code[X.error[0]], X.error[1]), (mode, X.error)
            ok = np.ones(n, dtype=bool)
            ok[X.row_type | X.row_index | X.row_range] = False
            assert np.array_equal(got[ok], X.out[ok]), mode             # the clean rows around the offender
        assert seen is None or seen == X.error                         # (both forms of the model agree)
        seen = X.error
    if want_error != 'any':
        assert seen == want_error, seen
    return seen


def test_bytes_0_and_255_pass_and_one_past_is_a_range_error(kernel):
    S2 = 16
    seq, qual, oq, meta = _clean(17, 16, 16, S2)
    fwd = [k for k in range(17) if not k & 1]
    seq[fwd[2], :2] = ord('A')                                          # AA at j = 1: byte 0; j = 0 has no context: byte 255
    X = P.analyse(seq, qual, oq, meta, P.int_probes(1, S2)['context'])
    assert X.out.min() == 0 and X.out.max() == 255
    _expect(kernel, (seq, qual, oq, meta), P.int_probes(1, S2)['context'], want_error=None)
    # one past: only the row whose base has quality 31 meets the moved cell
    row = fwd[2]
    for end, j, col in (('low', 1, 1), ('high', 0, 0)):
        q2 = qual.copy()
        q2[row, j] = 33 + CELL_Q
        assert (meta[row] >> 31) == 0
        model = P.one_past(1, S2, 0, CELL_Q, col, end)
        _expect(kernel, (seq, q2, oq, meta), model, want_error=(P.RangeError, row))
        assert P.analyse(seq, q2, oq, meta, model).out[row, j] == (-1 if end == 'low' else 256)
    # the float rows: totals next to the ends of the byte range, and far outside int32
    for total, error in ((-33.999999, None), (-34.0, (P.RangeError, row)), (222.999999, None), (223.0, (P.RangeError, row)),
                         (2.0e9, (P.RangeError, row)), (-2.0e9, (P.RangeError, row))):
        q2 = qual.copy()
        q2[row, 3] = 33 + CELL_Q
        model = P.float_cell(1, S2, 0, CELL_Q, 3, total)
        _expect(kernel, (seq, q2, oq, meta), model, want_error=error)
        if error is None:
            assert P.analyse(seq, q2, oq, meta, model, 6, 'f64').out[row, 3] == (0 if total < 0 else 255)


def test_index_errors(kernel):
    """The base at j = S2 (rows of 24 bases under 16 columns), for both strands and both mates; the same base below minscore;
    a quality with no model row."""
    S2, L = 16, 24
    model = P.int_probes(1, S2)['col161']
    clean = _clean(17, 32, L, S2)
    _expect(kernel, clean, model, want_error=None)
    for row in (8, 9, 10, 11):                                          # forward / reverse x first / second
        seq, qual, oq, meta = (x.copy() for x in clean)
        i = _i(meta[row], S2)
        assert i == (S2 if not row & 1 else L - 1 - S2)
        qual[row, i] = 33 + 6
        _expect(kernel, (seq, qual, oq, meta), model, want_error=(IndexError, row))
        qual[row, i] = 33 + 5                                           # below minscore: kept, no error
        _expect(kernel, (seq, qual, oq, meta), model, want_error=None)
        oq[row, i] = 33 + 42                                            # (the context plane is not the source)
        _expect(kernel, (seq, qual, oq, meta), model, want_error=None)
    seq, qual, oq, meta = (x.copy() for x in clean)
    qual[12, 5] = 33 + P.K.QT
    _expect(kernel, (seq, qual, oq, meta), model, want_error=(IndexError, 12))
    qual[12, 5] = 33 + P.K.QT - 1
    _expect(kernel, (seq, qual, oq, meta), model, want_error=None)


def test_type_errors(kernel):
    S2 = 16
    model = P.int_probes(1, S2)['context']
    clean = _clean(17, 16, 16, S2)
    R_ = ord('R')

    def case(row, edit, error):
        seq, qual, oq, meta = (x.copy() for x in clean)
        edit(seq, qual, oq)
        _expect(kernel, (seq, qual, oq, meta), model, want_error=(TypeError, row) if error else None)
    fwd, rev = 8, 9

    def put(plane, row, j, value):
        plane[row, _i(clean[3][row], j)] = value
    # an IUPAC letter as the previous base of j = 1
    case(fwd, lambda s, q, o: put(s, fwd, 0, R_), True)
    # ... as the current base, context quality 6, source quality below minscore
    case(fwd, lambda s, q, o: (put(s, fwd, 5, R_), put(s, fwd, 6, ord('N')), put(o, fwd, 5, 33 + 6), put(q, fwd, 5, 33 + 2)), True)
    # no error: at j = 0 as the current base only, the next base an N, or its context quality below 6
    case(fwd, lambda s, q, o: (put(s, fwd, 0, R_), put(s, fwd, 1, ord('N'))), False)
    case(fwd, lambda s, q, o: (put(s, fwd, 0, R_), put(o, fwd, 1, 33 + 5)), False)
    # context quality 5 (of the letter and of the base after it)
    case(fwd, lambda s, q, o: (put(s, fwd, 5, R_), put(o, fwd, 5, 33 + 5), put(o, fwd, 6, 33 + 5)), False)
    case(fwd, lambda s, q, o: (put(s, fwd, 5, R_), put(o, fwd, 5, 33 + 5)), True)          # (the base after it still looks it up)
    # the pairs RN and NR
    case(fwd, lambda s, q, o: (put(s, fwd, 5, R_), put(s, fwd, 4, ord('N')), put(s, fwd, 6, ord('N'))), False)
    # anywhere on a reverse row, where it becomes an N
    for j in (0, 1, 5, 15):
        case(rev, lambda s, q, o: put(s, rev, j, R_), False)


def test_precedence_and_the_first_offending_row(kernel):
    S2, L = 16, 24
    low = P.one_past(1, S2, 0, CELL_Q, 1, 'low')                       # AA at j = 1 with quality 31: byte -1
    clean = _clean(17, 32, L, S2, phase=3)

    def offend(planes_, row, what):
        seq, qual, oq, meta = planes_
        assert meta[row] >> 30 == 0                                     # forward, first mate
        if 'range' in what:
            seq[row, :2] = ord('A')
            qual[row, 1] = 33 + CELL_Q
        if 'index' in what:
            qual[row, S2] = 33 + Q
        if 'type' in what:
            seq[row, 9] = ord('R')
    # one row with all three
    planes_ = tuple(x.copy() for x in clean)
    offend(planes_, 9, 'range index type')
    X = P.analyse(*planes_, low)
    assert X.row_type[9] and X.row_index[9] and X.row_range[9]
    _expect(kernel, planes_, low, want_error=(TypeError, 9))
    planes_ = tuple(x.copy() for x in clean)
    offend(planes_, 9, 'range index')
    _expect(kernel, planes_, low, want_error=(IndexError, 9))
    # rows 5, 9 and 13 with Range, Index and Type: the first row decides, whatever its error
    for order in (('range', 'index', 'type'), ('index', 'type', 'range'), ('type', 'range', 'index')):
        planes_ = tuple(x.copy() for x in clean)
        for row, what in zip((5, 9, 13), order):
            offend(planes_, row, what)
        want = {'range': P.RangeError, 'index': IndexError, 'type': TypeError}[order[0]]
        _expect(kernel, planes_, low, want_error=(want, 5))
    # the offender in the last row and last chunk of a batch whose final workgroup has one live lane
    n = 257
    seq, qual, oq, meta = _clean(n, 16, 16, S2)
    assert meta[n - 1] >> 30 == 0
    seq[n - 1, :2] = ord('A')
    qual[n - 1, 1] = 33 + CELL_Q
    _expect(kernel, (seq, qual, oq, meta), low, want_error=(P.RangeError, n - 1))
    seq[n - 1, 15] = ord('R')
    _expect(kernel, (seq, qual, oq, meta), low, want_error=(TypeError, n - 1))


# ---------------------------------------------------------------------------------------------------- the quantize map
@pytest.mark.parametrize('key', ['p48', 'qt95'])
def test_the_map_meets_new_bytes_only(kernel, planes, key):
    """A map that is NOT the identity below 33 + minscore (a permutation of all 256 bytes): a preserved byte comes back as it
    was, a new byte comes back mapped, padding stays 0."""
    s = P.SHAPES[key]
    host = planes(key)
    d = [kernel.up(x) for x in host]
    table = ((7 * np.arange(256) + 13) % 256).astype(np.uint8)         # a bijection without a fixed point
    assert table[0] != 0 and (table != np.arange(256)).all()
    d_table = kernel.up(table)
    S2 = s.S2s[0]
    for name, model, mode, how in P.models(key, S2):
        if name not in ('col161', 'near', 'context'):
            continue
        blob = kernel.blob(model, mode, how)
        for minscore in s.minscores:
            X = P.analyse(*host, model, minscore, mode)
            new = P.aligned(X, X.use)
            want = np.where(new, table[X.out], X.out)
            assert (minscore == 0 or (~new & (X.out > 0)).any()) and (want != X.out).any()
            got, status, row = kernel.run(d, s.n, s.pitch, blob, minscore, qmap=d_table)
            assert (status, row) == (kernel.N.KBBQ_OK, -1)
            _same(got, want, '%s, %s, minscore %d' % (key, name, minscore))


# ---------------------------------------------------------------------------------------------------- the batch path
def _planes_of_sam(text, rg_to_int, use_oq):
    """Planes and row words from SAM text, by the header's words alone: (seq, qual, oq, meta, passthrough, lengths)."""
    recs = [ln.split('\t') for ln in text.splitlines() if ln and not ln.startswith('@')]
    pitch = max(16, (max(len(r[9]) for r in recs) + 15) // 16 * 16)
    n = len(recs)
    seq, qual, oq = (np.zeros((n, pitch), dtype=np.uint8) for _ in range(3))
    meta = np.zeros(n, dtype=np.uint32)
    passthrough = np.zeros(n, dtype=bool)
    for k, r in enumerate(recs):
        flag, L = int(r[1]), len(r[9])
        tags = dict((t[:2], t[5:]) for t in r[11:])
        seq[k, :L] = np.frombuffer(r[9].encode(), dtype=np.uint8)
        qual[k, :L] = np.frombuffer(r[10].encode(), dtype=np.uint8)
        if 'OQ' in tags:
            oq[k, :L] = np.frombuffer(tags['OQ'].encode(), dtype=np.uint8)
        passthrough[k] = use_oq and 'OQ' not in tags
        meta[k] = ((0 if passthrough[k] else L) | (rg_to_int[tags['RG']] << 16) | (int(use_oq) << 28) | (int('OQ' in tags) << 29)
                   | (int(bool(flag & 16)) << 30) | (int(bool(flag & 128)) << 31))
    return seq, qual, oq, meta, passthrough, np.array([len(r[9]) for r in recs])


@pytest.mark.parametrize('use_oq', [True, False])
def test_the_batch_path_writes_the_row_words(dev, tmp_path, use_oq):
    """applybqsr.recalibrate_alignments on a SAM and a BAM file of random alignments under the column and context probes."""
    import bamwriter
    from kbbq import aln
    from kbbq.gatk import applybqsr
    from test_gpu_applybqsr import _random_sam
    sam = _random_sam(tmp_path / 'r.sam', seed=23 + use_oq)
    text = open(sam).read()
    rg_to_int = {'g0': 0, 'g1': 1, 'g2': 2}
    seq, qual, oq, meta, passthrough, lens = _planes_of_sam(text, rg_to_int, use_oq)
    assert len(set((meta >> 28).tolist())) >= 6
    inside = np.arange(seq.shape[1])[None, :] < lens[:, None]
    probes = P.int_probes(3, 80)
    for name in ('col161', 'col157', 'context'):
        want = P.reference_apply(seq, qual, oq, meta, probes[name])
        want[passthrough] = qual[passthrough]
        for source in (sam, bamwriter.write_bam(tmp_path / ('%s.bam' % name), text)):
            got, off = applybqsr.recalibrate_alignments(aln.AlignmentFile(source), *probes[name], rg_to_int, use_oq=use_oq)
            assert applybqsr.LAST_RUN['mode'] == 'lut'
            assert np.array_equal(got, want[inside] - 33), name
            assert np.array_equal(np.diff(off), lens)


# ---------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_launch_nothing(kernel, planes):
    N = kernel.N
    s = P.SHAPES['p48']
    d = [kernel.up(x) for x in planes('p48')]
    model = P.int_probes(s.R, 96)['col161']
    d_lut, _, R, Qt, S2 = kernel.blob(model, 'lut')
    d_rows = kernel.blob(model, 'f64', 'rows')[0]
    d_out = kernel.T.full((s.n, s.pitch), 0xEE, dtype=kernel.T.uint8, device='cuda')

    def call(oq=N.ptr(d[2]), blob=N.ptr(d_lut), mode=N.ALIGNED_LUT, Qt=Qt):
        return kernel.lib.kbbq_apply_aligned_dev(kernel.ctx.handle, N.ptr(d[0]), N.ptr(d[1]), oq, N.ptr(d[3]), s.n, s.pitch, R, Qt, S2,
                                                 6, blob, mode, N.ptr(d_out))
    assert call(oq=ctypes.c_void_p(d[2].data_ptr() + 8)) == N.KBBQ_E_ARG
    assert call(blob=ctypes.c_void_p(d_lut.data_ptr() + 8)) == N.KBBQ_E_ARG
    assert call(mode=2) == N.KBBQ_E_ARG
    assert call(Qt=96) == N.KBBQ_E_ARG
    assert call(blob=N.ptr(d_rows), mode=N.ALIGNED_F64, Qt=224) == N.KBBQ_E_ARG
    assert kernel.status() == (N.KBBQ_OK, -1)
    assert (d_out.cpu().numpy() == 0xEE).all()
    assert call() == N.KBBQ_OK and kernel.status() == (N.KBBQ_OK, -1) and not (d_out.cpu().numpy() == 0xEE).any()
