"""kbbq_kmer_correct_rows_skip_dev on the MI355X (km_correct / km_correct_passes with TALLY): the corrected plane and counts of
kbbq_kmer_correct_rows_passes_dev byte for byte, and beside them the tally plane -- the rows' qualities with byte 0 at every
base the CPU model of the repeated rule (tests/kmer_passes_model.py) classes 2 -- in every layout the recalibrate path keeps
reads in: character rows, 4-bit one-read rows, mate-pair rows, twin rows and rows grouped by read group.  The model runs once
per (read set, k, N rule) on the reads one to a row; a row of two reads is its two reads side by side, separator and padding
class 0 (they are breaks)."""
import numpy as np
import pytest

import kmer_model as M
import kmer_passes_model as PM

pytestmark = pytest.mark.gpu

SECOND = np.uint32(1 << 31)
JUNK = 0xAA

_memo = {}


def _host(t):
    return t.cpu().numpy()


def _with_ns(seq, meta, seed, every=400):
    """`seq` with an N written over one base in `every` inside the reads (beside the few the generator leaves)."""
    rng = np.random.default_rng(seed)
    seq = seq.copy()
    inside = np.arange(seq.shape[1])[None, :] < (meta.astype(np.int64) & 0xFFFF)[:, None]
    seq[inside & (rng.random(seq.shape) < 1.0 / every)] = PM.NCH
    return seq


def _reads(name):
    """(seq, meta, qual) of a read set, made once: 'mixed' 36..300 bases, 'fixed' 100 bases (an odd number of reads)."""
    if name not in _memo:
        if name == 'mixed':
            seq, meta = M.synth(7, genome_len=8000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
        else:
            seq, meta = M.synth(5, genome_len=6000, depth=30, err=0.01, len_lo=100, len_hi=100)[:2]
            seq, meta = seq[:1799], meta[:1799]
        seq = _with_ns(seq, meta, 17)
        qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
        qual[np.arange(seq.shape[1])[None, :] >= (meta.astype(np.int64) & 0xFFFF)[:, None]] = 0
        for a in (seq, meta, qual):
            a.setflags(write=False)
        _memo[name] = (seq, meta, qual)
    return _memo[name]


def _model(name, k, fix_n):
    """(steps of PM.trace to 3 passes, t) of a read set, one read to a row: computed once and left unchanged."""
    key = (name, k, fix_n)
    if key not in _memo:
        seq, meta, _ = _reads(name)
        solid, t = PM.solid_set(seq, meta, k)
        steps = PM.trace(seq, meta, k, t, 3, fix_n=fix_n, solid_keys=solid)
        for step in steps:
            for a in step:
                a.setflags(write=False)
        _memo[key] = (steps, t)
    return _memo[key]


def _batch(seq, meta, qual):
    from kbbq import _device as dev
    return dev.ReadBatch.from_host(np.array(seq), np.array(qual), np.array(meta, dtype=np.uint32))


def _wide(plane, pitch):
    out = np.zeros((plane.shape[0], pitch), dtype=plane.dtype)
    w = min(pitch, plane.shape[1])
    out[:, :w] = plane[:, :w]
    return out


def _pair_rows(cls, changed, S, nrows, pitch):
    """The class plane and the changed counts of rows of two reads of S bases from those of the reads one to a row."""
    rows = np.zeros((nrows, pitch), dtype=np.uint8)
    per_row = np.zeros(nrows, dtype=np.int64)
    first, second = cls[0::2], cls[1::2]
    rows[:first.shape[0], :S] = first[:, :S]
    rows[:second.shape[0], S + 1:2 * S + 1] = second[:, :S]
    per_row[:first.shape[0]] += changed[0::2]
    per_row[:second.shape[0]] += changed[1::2]
    return rows, per_row


def _both_calls(table, batch, t, opts, passes):
    """(out, changed) of kbbq_kmer_correct_rows_passes_dev and (out, changed, tally, unresolved) of the skip call on a tally
    plane filled with JUNK, as host arrays; the batch's planes are left as they were."""
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    lib, ctx = N.load(), table.ctx
    n, pitch, flags = batch.n, batch.pitch, dev._row_flags(batch)
    seq_was, qual_was = _host(batch.seq).copy(), _host(batch.qual).copy()
    res = []
    for skip in (False, True):
        out = torch.full_like(batch.seq, JUNK)
        changed = torch.full((n,), -1, dtype=torch.int32, device='cuda')
        args = (ctx.handle, table.handle, N.ptr(batch.seq), N.ptr(batch.meta), n, pitch, flags, int(t), N.ptr(out), N.ptr(changed),
                opts, passes)
        if skip:
            tally = torch.full_like(batch.qual, JUNK)
            unres = torch.full((n,), -1, dtype=torch.int32, device='cuda')
            N.check(lib.kbbq_kmer_correct_rows_skip_dev(*args, N.ptr(batch.qual), N.ptr(tally), N.ptr(unres)))
            ctx.status()
            res.append((_host(out), _host(changed), _host(tally), _host(unres).astype(np.int64)))
        else:
            N.check(lib.kbbq_kmer_correct_rows_passes_dev(*args))
            ctx.status()
            res.append((_host(out), _host(changed)))
    assert np.array_equal(_host(batch.seq), seq_was) and np.array_equal(_host(batch.qual), qual_was)
    return res[0], res[1], qual_was


def _check(table, batch, t, opts, passes, cls, changed):
    """Both calls on `batch` against the model's class plane [rows, pitch] and changed counts per row of the batch."""
    plain, skip, qual = _both_calls(table, batch, t, opts, passes)
    n = batch.n
    assert cls.shape == qual[:n].shape == (n, batch.pitch)
    assert np.array_equal(skip[0], plain[0]) and np.array_equal(skip[1], plain[1])         # d_out, d_changed: byte for byte
    assert np.array_equal(plain[1][:n].astype(np.int64), changed)
    want = np.where(cls == 2, 0, qual[:n]).astype(np.uint8)
    assert np.array_equal(skip[2][:n], want)                                                # the whole plane, padding included
    assert np.array_equal(skip[3][:n], (cls == 2).sum(axis=1))
    again = _both_calls(table, batch, t, opts, passes)[1]
    assert all(np.array_equal(a, b) for a, b in zip(skip, again))                           # two runs: the same planes
    return int((cls == 2).sum())


def test_the_model_has_unresolved_bases_to_skip():
    """Vacuity guard: the mixed set at k = 31 has a class-2 share of at least 0.02 after one pass (the model gives 0.0868) and
    above 0 after three."""
    seq, meta, _ = _reads('mixed')
    steps, _ = _model('mixed', 31, False)
    bases = int((meta & 0xFFFF).sum())
    one, three = (int((steps[P - 1][2] == 2).sum()) / bases for P in (1, 3))
    print('class-2 share of the mixed set at k = 31: %.4f after one pass, %.4f after three' % (one, three))
    assert one >= 0.02 and 0 < three < one


@pytest.mark.parametrize('layout', ('reads', 'reads_nib'))
def test_hand_built_rows(layout):
    from kbbq import _device as dev
    from kbbq import kmer
    seq, meta, cases = PM.hand_rows()
    assert seq.shape[1] == 48
    qual = (np.random.default_rng(4).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    qual[np.arange(48)[None, :] >= meta.astype(np.int64)[:, None]] = 0
    steps = PM.trace(seq, meta, PM.HAND_K, PM.HAND_T, 4)
    twos = [int((s[2] == 2).sum()) for s in steps]
    assert twos[0] > 0 and len({s[2].tobytes() for s in steps[:3]}) == 3       # the passes differ in what they leave unresolved
    batch = _batch(seq, meta, qual)
    if layout == 'reads_nib':
        batch = dev.lay_out(batch, 1, pairs=False)
    assert batch.layout_key() == layout and batch.n == seq.shape[0]
    table = kmer.count_batch(batch, k=PM.HAND_K)
    try:
        for P in (1, 2, 3, 4):
            _check(table, batch, PM.HAND_T, 0, P, _wide(steps[P - 1][2], batch.pitch), steps[P - 1][1])
    finally:
        table.close()


@pytest.mark.parametrize('cut, pitch', ((PM.HAND_K, 48), (PM.HAND_K - 1, 48), (PM.HAND_K, 16)))
@pytest.mark.parametrize('layout', ('reads', 'reads_nib'))
def test_reads_of_k_and_of_k_minus_1_bases(layout, cut, pitch):
    """Edge rows: every read has exactly one window, or none (nothing is unresolved: the tally plane is the quality plane); at
    pitch 48 the rows are wider than the longest read."""
    from kbbq import _device as dev
    from kbbq import kmer
    seq, meta, _ = PM.hand_rows(pitch=pitch, cut=cut)
    qual = np.full(seq.shape, 33 + 30, dtype=np.uint8)
    qual[:, cut:] = 0
    steps = PM.trace(seq, meta, PM.HAND_K, PM.HAND_T, 2)
    if cut < PM.HAND_K:
        assert not steps[1][2].any()
    batch = _batch(seq, meta, qual)
    if layout == 'reads_nib':
        batch = dev.lay_out(batch, 1, pairs=False)
    assert batch.layout_key() == layout
    table = kmer.count_batch(batch, k=PM.HAND_K)
    try:
        for P in (1, 2):
            _check(table, batch, PM.HAND_T, 0, P, _wide(steps[P - 1][2], batch.pitch), steps[P - 1][1])
    finally:
        table.close()


def _laid(layout):
    """(batch, how the model's planes of the reads become the batch's rows) for a layout of the recalibrate path."""
    from kbbq import _device as dev
    name = 'mixed' if layout in ('reads', 'reads_nib', 'grouped') else 'fixed'
    seq, meta, qual = _reads(name)
    meta = np.array(meta)
    if layout == 'reads':
        batch = _batch(seq, meta, qual)
    elif layout == 'reads_nib':
        batch = dev.lay_out(_batch(seq, meta, qual), 1)
    elif layout == 'grouped':
        meta |= np.random.default_rng(5).integers(0, 3, meta.size).astype(np.uint32) << np.uint32(16)
        batch = dev.lay_out(_batch(seq, meta, qual), 3)
        assert batch.seg is not None and batch.perm is not None
    elif layout in ('pairs', 'pairs_nib'):
        seq, meta, qual = seq[:-1], meta[:-1], qual[:-1]
        meta[1::2] |= SECOND
        batch = dev.lay_out(_batch(seq, meta, qual), 1, packed=layout == 'pairs_nib')
        assert not batch.twins and batch.n == seq.shape[0] // 2
    else:
        assert seq.shape[0] % 2 == 1                         # the last row's second half is padding
        batch = dev.lay_out(_batch(seq, meta, qual), 1)
        assert batch.twins and batch.n == (seq.shape[0] + 1) // 2
    want_key = {'grouped': 'reads_nib', 'twins': 'pairs_nib'}.get(layout, layout)
    assert batch.layout_key() == want_key
    nreads = seq.shape[0]

    def rows(step):
        cls, changed = step[2][:nreads], step[1][:nreads]
        if layout in ('reads', 'reads_nib'):
            return _wide(cls, batch.pitch), changed
        if layout == 'grouped':
            perm = _host(batch.perm)[:batch.n]
            assert not np.array_equal(perm, np.arange(perm.size))
            return _wide(cls[perm], batch.pitch), changed[perm]
        return _pair_rows(cls, changed, 100, batch.n, batch.pitch)
    return name, batch, rows


@pytest.mark.parametrize('k', (31, 15))
@pytest.mark.parametrize('layout', ('reads', 'reads_nib', 'pairs', 'pairs_nib', 'twins', 'grouped'))
def test_layouts_equal_the_model(layout, k):
    from kbbq import _native as N
    from kbbq import kmer
    name, batch, rows = _laid(layout)
    table = kmer.count_batch(batch, k=k)
    try:
        twos = {}
        for fix_n in (False, True):
            steps, t = _model(name, k, fix_n)
            for P in (1, 3):
                cls, changed = rows(steps[P - 1])
                twos[fix_n, P] = _check(table, batch, t, N.KMER_FIX_N if fix_n else 0, P, cls, changed)
        # the case has something to skip, fewer after three passes, and the N rule changes what is decided
        assert twos[False, 1] > twos[False, 3] > 0
        assert int(_model(name, k, True)[0][0][1].sum()) > int(_model(name, k, False)[0][0][1].sum())
    finally:
        table.close()


def test_refusals_write_nothing():
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta, _ = PM.hand_rows()
    qual = np.full(seq.shape, 33 + 30, dtype=np.uint8)
    batch = _batch(seq, meta, qual)
    lib, ctx = N.load(), dev.context()
    table = kmer.count_batch(batch, k=PM.HAND_K)
    try:
        n, pitch = batch.n, batch.pitch
        out = torch.full_like(batch.seq, JUNK)
        tally = torch.full_like(batch.qual, JUNK)
        counts = torch.full((2, n), JUNK, dtype=torch.int32, device='cuda')
        qual_was = _host(batch.qual).copy()

        def call(opts=0, passes=1, d_qual=N.ptr(batch.qual), d_tally=N.ptr(tally), flags=0, min_count=PM.HAND_T):
            return lib.kbbq_kmer_correct_rows_skip_dev(ctx.handle, table.handle, N.ptr(batch.seq), N.ptr(batch.meta), n, pitch, flags,
                                                       min_count, N.ptr(out), N.ptr(counts[0]), opts, passes, d_qual, d_tally,
                                                       N.ptr(counts[1]))
        for kw, word in ((dict(d_qual=None), 'd_qual'), (dict(d_tally=None), 'd_tally_qual'),
                         (dict(d_tally=N.ptr(batch.qual)), 'd_tally_qual is d_qual'),
                         (dict(opts=N.KMER_FLAG_UNRESOLVED), 'opts'), (dict(opts=N.KMER_FLAG_UNRESOLVED | N.KMER_FIX_N), 'opts'),
                         (dict(opts=4), 'opts'), (dict(opts=8 | N.KMER_FIX_N), 'opts'),
                         # ... and those of kbbq_kmer_correct_rows_passes_dev
                         (dict(passes=0), 'passes'), (dict(passes=9), 'passes'), (dict(flags=8), 'flags'),
                         (dict(flags=N.ROWS_TWINS), 'TWINS'), (dict(min_count=0), 'min_count'),
                         (dict(d_tally=N.ptr(tally.view(-1)[4:])), 'aligned')):
            assert call(**kw) == N.KBBQ_E_ARG, kw
            assert word in N.last_error(), (kw, N.last_error())
        ctx.status()
        assert int((out != JUNK).sum()) == 0 and int((tally != JUNK).sum()) == 0 and int((counts != JUNK).sum()) == 0
        assert np.array_equal(_host(batch.qual), qual_was)
        # no rows: nothing is launched
        assert lib.kbbq_kmer_correct_rows_skip_dev(ctx.handle, table.handle, N.ptr(batch.seq), N.ptr(batch.meta), 0, pitch, 0, PM.HAND_T,
                                                   N.ptr(out), N.ptr(counts[0]), 0, 2, N.ptr(batch.qual), N.ptr(tally),
                                                   N.ptr(counts[1])) == N.KBBQ_OK
        ctx.status()
        assert int((out != JUNK).sum()) == 0 and int((tally != JUNK).sum()) == 0 and int((counts != JUNK).sum()) == 0
        # the context and the table go on working, d_unresolved may be NULL
        steps = PM.trace(seq, meta, PM.HAND_K, PM.HAND_T, 2)
        assert lib.kbbq_kmer_correct_rows_skip_dev(ctx.handle, table.handle, N.ptr(batch.seq), N.ptr(batch.meta), n, pitch, 0, PM.HAND_T,
                                                   N.ptr(out), N.ptr(counts[0]), 0, 2, N.ptr(batch.qual), N.ptr(tally), None) == N.KBBQ_OK
        ctx.status()
        assert np.array_equal(_host(tally), np.where(steps[1][2] == 2, 0, qual_was))
        assert np.array_equal(_host(counts[0]).astype(np.int64), steps[1][1]) and int((counts[1] != JUNK).sum()) == 0
    finally:
        table.close()


def test_correct_batch_keyword():
    """kmer.correct_batch(skip_unresolved=True): the batch's tally plane in its own layout and the per-row unresolved counts
    beside the changed counts; without the keyword the return is the array it was and the batch gets no tally plane."""
    from kbbq import kmer
    name, batch, rows = _laid('pairs_nib')
    steps, t = _model(name, 31, False)
    cls, changed = rows(steps[0])
    table = kmer.count_batch(batch, k=31)
    try:
        plain = kmer.correct_batch(table, batch, t)
        assert not isinstance(plain, tuple) and batch.tally_qual is None
        cseq = _host(batch.cseq).copy()
        got_changed, got_unres = kmer.correct_batch(table, batch, t, skip_unresolved=True)
        assert np.array_equal(_host(batch.cseq), cseq) and np.array_equal(_host(got_changed), _host(plain))
        assert np.array_equal(_host(got_changed).astype(np.int64), changed)
        assert np.array_equal(_host(got_unres).astype(np.int64), (cls == 2).sum(axis=1))
        assert batch.tally_qual.shape == batch.qual.shape and batch.tally_qual.data_ptr() != batch.qual.data_ptr()
        assert np.array_equal(_host(batch.tally_qual)[:batch.n], np.where(cls == 2, 0, _host(batch.qual)[:batch.n]))
    finally:
        table.close()
