"""
CPU tests of tests/aligned_apply_probe.py, which the GPU tests of the aligned ApplyBQSR kernel (test_gpu_aligned_apply_probe.py)
rest on:
  * `reference_apply` is anchored to the real reference: the goldens' `ab_recal`, and the per-read port recalibrate_bamread on
    random alignments, from the planes and row words the product's batch path builds;
  * the probes discriminate: on every shape, every index mistake of `MISTAKES` that can show there changes a byte under one of
    the models the GPU test runs on that shape -- a condition on probes and rows, not on any kernel;
  * the rows reach what the shapes are there for (contexts on both strands at a chunk's two ends and at a wave's two ends,
    every column, both sides of both thresholds, order-sensitive float cells), computed from the reference alone;
  * applybqsr._model chooses the form the probes expect and its blob is the model, cell by cell.
"""
import ctypes

import numpy as np
import pytest

import aligned_apply_probe as P

SEED = 0


@pytest.fixture(scope='module')
def planes():
    made = {}

    def get(key):
        if key not in made:
            made[key] = P.rows(key, SEED)
            for x in made[key]:
                x.setflags(write=False)
        return made[key]
    return get


# ---------------------------------------------------------------------------------------------------- the anchor
def _batch_planes(bam, rg_to_int, R, use_oq):
    """Planes and row words as the batch path hands them to the kernel (applybqsr._recalibrated_slabs)."""
    from kbbq.gatk import applybqsr
    b = bam.batch()
    n = len(bam)
    pitch = max(16, (int(b.maxlen) + 15) // 16 * 16)
    meta, passthrough = applybqsr._rows(bam, rg_to_int, R, use_oq, 0, n)
    return b.plane(0, pitch, 0, n), b.plane(1, pitch, 0, n), b.plane(2, pitch, 0, n), meta, passthrough, b


def _flat(out, lens):
    return out[np.arange(out.shape[1])[None, :] < lens[:, None]] - 33


@pytest.mark.parametrize('name', ['bqsr_a', 'bqsr_b'])
def test_the_reference_reproduces_the_goldens(oracle, name, tmp_path):
    from kbbq import aln, compare_reads
    from test_oracle_bqsr import VEC, _inputs
    _, gold, paths = _inputs(name, tmp_path, oracle)
    vectors = [gold[k] for k in VEC]
    model = (vectors[0],) + tuple(oracle.get_delta_qs(*vectors))
    bam = aln.AlignmentFile(paths['sam'])
    rg_to_int = {rg: i for i, rg in enumerate(compare_reads.get_rg_to_pu(bam))}
    seq, qual, oq, meta, passthrough, b = _batch_planes(bam, rg_to_int, len(model[0]), True)
    assert not passthrough.any()
    mode = 'lut' if all(np.asarray(x).dtype.kind in 'iu' for x in model) else 'f64'
    out = P.reference_apply(seq, qual, oq, meta, model, 6, mode)
    assert np.array_equal(_flat(out, b.qlen.astype(np.int64)), gold['ab_recal'])
    assert set(((meta >> 30) & 1).tolist()) == {0, 1} == set((meta >> 31).tolist())          # both strands, both mates


@pytest.mark.parametrize('use_oq', [True, False])
@pytest.mark.parametrize('kind', ['int', 'float'])
def test_the_reference_is_the_per_read_function(tmp_path, use_oq, kind):
    from kbbq import aln
    from test_gpu_applybqsr import _host_reference, _random_model, _random_sam
    sam = _random_sam(tmp_path / 'r.sam', seed=5 + use_oq)
    model = _random_model(7, 3, 40, kind)
    rg_to_int = {'g0': 0, 'g1': 1, 'g2': 2}
    bam = aln.AlignmentFile(sam)
    seq, qual, oq, meta, passthrough, b = _batch_planes(bam, rg_to_int, 3, use_oq)
    out = P.reference_apply(seq, qual, oq, meta, model, 6, 'lut' if kind == 'int' else 'f64')
    out[passthrough] = qual[passthrough]
    lens = np.where(passthrough, b.qual_len, b.qlen).astype(np.int64)
    want = _host_reference(aln.AlignmentFile(sam), model, rg_to_int, use_oq)
    assert np.array_equal(_flat(out, lens), want)
    assert passthrough.any() == use_oq and (want < 6).any()


def test_the_reference_names_the_error_and_the_row():
    """Type, then Index, then Range within a row; the first offending row across rows; what is NOT an error."""
    n, pitch, S2 = 16, 16, 8
    model = P.int_probes(1, S2)['context']

    def batch():
        seq = np.zeros((n, pitch), dtype=np.uint8)
        seq[:, :8] = np.frombuffer(b'ACGTTGCA', dtype=np.uint8)
        qual = np.zeros((n, pitch), dtype=np.uint8)
        qual[:, :8] = 33 + 30
        return seq, qual, np.full(n, 8, dtype=np.uint32)
    seq, qual, meta = batch()
    assert P.analyse(seq, qual, None, meta, model).error is None
    seq[13, 3] = ord('R')
    qual[9, 2] = 33 + 43
    low = P.one_past(1, S2, 0, 30, 1, 'low')                            # row 5: 'AA' at j = 1
    seq[5, :2] = ord('A')
    for m, want in ((model, (IndexError, 9)), (low, (P.RangeError, 5))):
        assert P.analyse(seq, qual, None, meta, m).error == want
        with pytest.raises(want[0]) as e:
            P.reference_apply(seq, qual, None, meta, m)
        assert e.value.row == want[1]
    qual[13, 2] = 33 + 43
    seq[13, :2] = ord('A')
    meta[[5, 9]] = 0
    X = P.analyse(seq, qual, None, meta, low)
    assert X.row_type[13] and X.row_index[13] and X.row_range[13] and X.error == (TypeError, 13)
    assert not X.out[5].any() and not X.out[9].any()                   # L = 0
    # no error: the letter next to an N, under context quality 5, as the current base of j = 0, or on a reverse row
    for edit, clean in ((lambda s, q, m: s.__setitem__((13, 4), ord('N')), False),       # R at 3: 'GR' is still looked up
                        (lambda s, q, m: (s.__setitem__((13, 2), ord('N')), s.__setitem__((13, 4), ord('N'))), True),
                        (lambda s, q, m: (q.__setitem__((13, 3), 33 + 5), q.__setitem__((13, 4), 33 + 5)), True),
                        (lambda s, q, m: m.__setitem__(13, 8 | (1 << 30)), True)):
        seq, qual, meta = batch()
        seq[13, 3] = ord('R')
        edit(seq, qual, meta)
        assert (P.analyse(seq, qual, None, meta, model).error is None) == clean
    seq, qual, meta = batch()
    seq[13, 0] = ord('R')
    assert P.analyse(seq, qual, None, meta, model).error == (TypeError, 13)       # as the previous base of j = 1
    seq[13, 1] = ord('N')
    assert P.analyse(seq, qual, None, meta, model).error is None
    # the current base's SOURCE quality does not matter to the TypeError, its CONTEXT quality does
    seq, qual, meta = batch()
    oq = qual.copy()
    seq[13, 3] = ord('R')
    seq[13, 4] = ord('N')
    qual[13, 3] = 33 + 2
    meta[13] |= 1 << 29                                                 # source QUAL (2), context OQ (30)
    assert P.analyse(seq, qual, oq, meta, model).error == (TypeError, 13)
    oq[13, 3] = 33 + 5
    assert P.analyse(seq, qual, oq, meta, model).error is None


# ---------------------------------------------------------------------------------------------------- discriminating power
_RIGHT = {}


def _right(key, planes, S2):
    """[(name, model, mode, minscore, the reference's bytes)] of shape `key`, made once."""
    if key not in _RIGHT:
        _RIGHT.clear()                                                  # (one shape's models at a time)
        made = []
        for name, model, mode, _ in P.models(key, S2):
            for minscore in P.SHAPES[key].minscores:
                right = P.analyse(*planes, model, minscore, mode)
                assert right.error is None, (key, name, right.error)
                made.append((name, model, mode, minscore, right))
        _RIGHT[key] = made
    return _RIGHT[key]


def _caught_by(key, planes, S2, wrong, first_only=True):
    """The (model name, minscore) under which mistake `wrong` changes a byte of shape `key`."""
    seen = []
    for name, model, mode, minscore, right in _right(key, planes, S2):
        if mode not in P.MISTAKES[wrong]:
            continue
        bad = P.analyse(*planes, model, minscore, mode, wrong)
        if bad.error is not None or not np.array_equal(bad.out, right.out):
            seen.append((name, minscore))
            if first_only:
                return seen
    return seen


@pytest.mark.parametrize('key', list(P.SHAPES))
def test_every_mistake_changes_a_byte_on_every_shape(planes, key):
    S2 = P.SHAPES[key].S2s[0]
    missed = []
    for wrong in P.MISTAKES:
        why = P.NOT_APPLICABLE.get((key, wrong))
        caught = _caught_by(key, planes(key), S2, wrong)
        if why is not None:
            assert not caught, '%s / %s is listed as not applicable (%s) but shows under %s' % (key, wrong, why, caught)
        elif not caught:
            missed.append(wrong)
    table = {w: _caught_by(key, planes(key), S2, w, first_only=False) for w in missed}
    assert not missed, '%s: no model of this shape sees %s' % (key, table)


def test_the_exceptions_are_the_listed_ones():
    assert all(k in P.SHAPES and w in P.MISTAKES and why for (k, w), why in P.NOT_APPLICABLE.items())
    f64_only = [w for w, modes in P.MISTAKES.items() if modes == ('f64',)]
    assert len(f64_only) == 3                                           # ... which no LUT model is asked about
    for key in P.SHAPES:
        assert any(mode == 'f64' for _, _, mode, _ in P.models(key, 16)) or key == 'qt95'


# ---------------------------------------------------------------------------------------------------- coverage
ALL = {(rev, ctx) for rev in (0, 1) for ctx in range(P.D)}
DINUC = {(rev, ctx) for rev in (0, 1) for ctx in range(16)}
# byte 0 of a forward row's first chunk and byte 15 of a reverse row's last chunk are j = 0: rows of one chunk have no
# dinucleotide there.  64 rows of 2 chunks, of which 24 have a second chunk, cannot hold 17 contexts per strand at it.
ONE_CHUNK = {'p16'}
TOO_FEW_CHUNKS = {'rg4096'}
# rows that straddle a wave edge (the chunks of a row do not divide 64) in a batch of more than a handful of waves; the
# 64 x 48 rows of the Qt shapes are three waves, whose one mid-row lane 63 sits on whatever strand the shuffle gave it.
# Those shapes, p16 and rg4096 still assert that lane 0 and lane 63 are looked up at byte 0 and at byte 15.
STRADDLE = {'p48', 'p160', 'p1040', 'long'}


@pytest.mark.parametrize('key', list(P.SHAPES))
def test_the_rows_reach_what_the_shape_is_for(planes, key):
    s = P.SHAPES[key]
    seq, qual, oq, meta = planes(key)
    L = meta.astype(np.int64) & 0xFFFF
    assert seq.shape == (s.n, s.pitch) and set(L.tolist()) == set(s.lengths)
    inside = np.arange(s.pitch)[None, :] < L[:, None]
    assert (qual != oq)[inside].all() and not seq[~inside].any() and not qual[~inside].any() and not oq[~inside].any()
    assert (seq[inside] == ord('N')).mean() > 0.04
    for S2 in s.S2s:
        for minscore in s.minscores:
            cov = P.coverage(key, planes(key), S2, minscore)
            assert cov['contexts'] == ALL
            if key == 'long':
                assert cov['strand x mate'] == {(0, 1), (1, 0), (1, 1)}            # three rows
            else:
                assert len(cov['strand x mate']) == 4 and cov['planes'] == {0, 1, 2, 3}
            if key in ONE_CHUNK:
                assert cov['byte', 0] == {(0, 16)} | {(1, c) for c in range(P.D)}
                assert cov['byte', 15] == {(1, 16)} | {(0, c) for c in range(P.D)}
            elif key not in TOO_FEW_CHUNKS:
                assert cov['byte', 0] == ALL and cov['byte', 15] == ALL
            if key == 'long':                                           # 192 waves: every context at every wave end
                for b in (0, 15):
                    for lane in (0, 63):
                        assert cov['byte', b, 'lane', lane] == ALL
            elif key in STRADDLE:
                # a handful of waves: the neighbour that comes from memory (forward: before lane 0; reverse: after lane 63)
                # is a dinucleotide's on both strands, and lane 0 / lane 63 are looked up at both ends of their chunk
                assert {r for r, c in cov['byte', 0, 'lane', 0] if c < 16} == {0, 1}
                assert {r for r, c in cov['byte', 15, 'lane', 63] if c < 16} == {0, 1}
            # whatever the number of waves: lane 0 and lane 63 are looked up at both ends of their chunk
            for b in (0, 15):
                for lane in (0, 63):
                    assert cov['byte', b, 'lane', lane], (b, lane)
            if S2 <= 320:
                top = max(s.lengths) if key != 'rg4096' else S2
                assert cov['columns'][0] == set(range(top)) and cov['columns'][1] == set(range(S2 - top, S2))
                assert cov['columns'][0] | cov['columns'][1] == set(range(S2))
            assert {5, 6} <= cov['context quality on a pair']
            assert minscore in cov['source quality'] and (minscore == 0 or minscore - 1 in cov['source quality'])
    assert P.runs_order_probe(key) == (key != 'qt95')                 # (the LUT form's shape has no F64 run)
    if P.runs_order_probe(key):
        for S2 in s.S2s:
            for minscore in s.minscores:
                n2, n3 = P.order_sensitive(planes(key), P.order_model(key, S2), minscore)
                assert n2 >= 100 and n3 >= 100, (S2, minscore, n2, n3)
        named = [m for name, m, _, _ in P.models(key, 16) if name.startswith('order')]
        assert len(named) == 1 and all(np.array_equal(a, b) for a, b in zip(named[0], P.order_model(key, 16)))


def test_counts_for_the_record(planes, capsys):
    """Looked-up bases, and bases that truncate differently under each of the two other summation orders, per shape and
    minscore (printed with -s)."""
    for key, s in P.SHAPES.items():
        for minscore in s.minscores:
            looked = P.coverage(key, planes(key), s.S2s[0], minscore)['looked up']
            sens = P.order_sensitive(planes(key), P.order_model(key, s.S2s[0]), minscore) if P.runs_order_probe(key) else 'no F64 run'
            print('%-7s minscore %2d: %6d looked-up bases, order-sensitive %s' % (key, minscore, looked, sens))
            assert looked > 500


# ---------------------------------------------------------------------------------------------------- the probe models
def test_the_integer_probes_keep_their_promises():
    for R, S2, Qt in ((3, 32, 43), (2, 96, 95), (2, 96, 223)):
        for name, model in P.int_probes(R, S2, Qt).items():
            cyc, ctx = P.K.entries(model)
            sums = cyc[:, :, :, None] + ctx[:, :, None, :] + 33
            assert sums.min() >= 0 and sums.max() <= 255, name
        cyc, ctx = P.K.entries(P.int_probes(R, S2, Qt)['context'])
        sums = cyc[:, :, :, None] + ctx[:, :, None, :] + 33
        assert sums.min() == 0 and sums.max() == 255
    for sign in (1, -1):
        cyc, ctx = P.K.entries(P.int16_ends(3, 320, sign))
        sums = cyc[:, :, :, None] + ctx[:, :, None, :] + 33
        assert sums.min() == 0 and sums.max() == 255
        assert np.abs(cyc).min() >= 31700 and np.abs(ctx).min() >= 31700 and np.abs(cyc).max() <= 32767 and np.abs(ctx).max() <= 32767
        assert (np.sign(cyc) == sign).all() and (np.sign(ctx) == -sign).all()


def test_the_int16_ends_go_through_build_lut(planes):
    """kbbq_build_lut takes them (KBBQ_OK) and _model hands out its blob; on the everyday rows the bytes 0 and 255 are reached."""
    from kbbq import _native as N
    from kbbq.gatk import applybqsr
    lib = N.load()
    for sign in (1, -1):
        model = P.int16_ends(3, 320, sign)
        a = [np.ascontiguousarray(x, dtype=np.int64) for x in model]
        blob = np.zeros((lib.kbbq_lut_bytes(3, 43, 320) + 15) // 16 * 16, dtype=np.uint8)
        flags = ctypes.c_int(0)
        rc = lib.kbbq_build_lut(3, 43, 320, 17, 6, *[N.ptr(x) for x in a], N.ptr(blob), ctypes.byref(flags))
        assert rc == N.KBBQ_OK
        mode, got, R, Qt, S2 = applybqsr._model(*model, 6)
        assert mode == N.ALIGNED_LUT and np.array_equal(got, blob)
        out = P.reference_apply(*planes('p160'), model)
        assert out.min() == 0 and out.max() == 255


def test_the_float_probes_sit_where_they_say():
    R, S2 = 3, 32
    r, q, ctx, col = (x.reshape(-1) for x in np.meshgrid(np.arange(R), np.arange(43), np.arange(17), np.arange(S2), indexing='ij'))
    for name, model in P.float_probes(R, S2).items():
        v, far = P._sum(model, 'f64', r, q, col, ctx)
        assert not far.any() and v.min() + 33 >= 0 and v.max() + 33 <= 255 and v.min() < 0, name
        floor, _ = P._sum(model, 'f64', r, q, col, ctx, 'F64: floor')
        assert (floor != v).sum() > 1000, name                        # totals below zero that are no integers
        m = [np.asarray(x, dtype=np.float64) for x in model]
        exact = ((m[0][r] + m[1][r]) + m[2][r, q] + m[4][r, q, ctx]) + m[3][r, q, col]
        assert (np.abs(exact - np.rint(exact)) < 2.0 ** -40).mean() > (0.99 if name == 'near' else 0.0)
    model = P.order_probe(R, S2)
    v, _ = P._sum(model, 'f64', r, q, col, ctx)
    v2, _ = P._sum(model, 'f64', r, q, col, ctx, 'F64: base + (dinuc + pos)')
    v3, _ = P._sum(model, 'f64', r, q, col, ctx, 'F64: (base + pos) + dinuc')
    base = (model[0][r] + model[1][r]) + model[2][r, q]
    high = base >= 16
    assert np.array_equal(v2 != v, high & P.ORDER_EVEN[ctx] & (col % 3 != 0))
    assert np.array_equal(v3 != v, high & ~P.ORDER_EVEN[ctx] & (col % 3 == 0))
    assert ((v2 != v) & (v3 == v)).any() and ((v3 != v) & (v2 == v)).any()
    for total, byte in ((-33.999999, 0), (-34.0, -1), (222.999999, 255), (223.0, 256), (2.0e9, None), (-2.0e9, None)):
        v, far = P._sum(P.float_cell(2, 16, 1, 30, 5, total), 'f64', *(np.array([x]) for x in (1, 30, 5, 3)))
        assert (far[0] and byte is None) or v[0] + 33 == byte


# ---------------------------------------------------------------------------------------------------- applybqsr._model
def _gather(mode, blob, R, Qt, S2, N, lib):
    """Every (rg, q, context, column) cell from the blob _model returns, as the kernel reads it."""
    if mode == N.ALIGNED_LUT:
        rs = lib.kbbq_lut_row_stride(S2)
        lut = blob[:R * Qt * rs * 2].view(np.int16).reshape(R, Qt, rs).astype(np.int64)
        five = np.array([5 * (c // 4) + c % 4 for c in range(16)] + [24])
        return lut[:, :, None, :S2] + lut[:, :, S2 + five][:, :, :, None]
    rows = blob.view(np.float64).reshape(R, Qt, 18 + S2)
    return np.trunc((rows[:, :, 0][:, :, None, None] + rows[:, :, 1:18, None]) + rows[:, :, None, 18:]).astype(np.int64)


def test_model_folding():
    from kbbq import _native as N
    from kbbq.gatk import applybqsr
    lib = N.load()
    R, S2 = 3, 20
    r, q, ctx, col = np.meshgrid(np.arange(R), np.arange(43), np.arange(17), np.arange(S2), indexing='ij')
    cases = [(name, m, N.ALIGNED_F64) for name, m in P.float_probes(R, S2).items()]
    cases += [(name + ' in float64', tuple(np.asarray(x, dtype=np.float64) for x in m), N.ALIGNED_LUT)
              for name, m in list(P.int_probes(R, S2).items()) + [('int16 +-', P.int16_ends(R, S2, 1))]]
    cases += [(name, m, N.ALIGNED_LUT) for name, m in P.int_probes(R, S2).items()]
    cases += [('223 rows', P.int_probes(R, S2, 223)['col161'], N.ALIGNED_F64)]
    for name, model, form in cases:
        mode, blob, R_, Qt, S2_ = applybqsr._model(*model, 6)
        assert (mode, R_, S2_) == (form, R, S2), name
        if Qt != 43:
            r, q, ctx, col = np.meshgrid(np.arange(R), np.arange(Qt), np.arange(17), np.arange(S2), indexing='ij')
        want, far = P._sum(model, 'f64', r, q, col, ctx)
        assert not far.any()
        assert np.array_equal(_gather(mode, blob, R, Qt, S2, N, lib), want), name
        if mode == N.ALIGNED_F64:
            assert np.array_equal(blob.view(np.float64).reshape(R, Qt, 18 + S2), P.f64_rows(model)), name
