"""The k-mer calls on device batches in the recalibrate path's layouts (kbbq.kmer count_batch / prefilter_batch / correct_batch,
kbbq_kmer_*_rows_dev) on the MI355X: 4-bit planes, mate-pair and twin rows, rows grouped by read group, rows of more than 256
chunks and character rows through the same calls, each against the CPU model (tests/kmer_model.py) run on the laid batch's own
characters and sidecar lengths -- a row of two reads is one row with a break in the model as on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECOND = np.uint32(1 << 31)


def _qual(seq, lens):
    q = np.full(seq.shape, 33 + 30, dtype=np.uint8)
    q[np.arange(seq.shape[1])[None, :] >= np.asarray(lens, dtype=np.int64)[:, None]] = 0
    return q


def _batch(seq, meta):
    from kbbq import _device as dev
    meta = np.asarray(meta, dtype=np.uint32)
    return dev.ReadBatch.from_host(np.ascontiguousarray(seq), _qual(seq, meta & 0xFFFF), meta)


def _rows(batch, name='seq'):
    """(characters [n, pitch], sidecar lengths) of a laid batch."""
    chars = batch.chars(name)[:batch.n].cpu().numpy()
    lens = batch.meta[:batch.n].cpu().numpy().view(np.uint32) & 0xFFFF
    return chars, lens


class _PlainIndices:
    """NumPy as kmer_model sees it, with nonzero() handing out Python ints: M.correct shifts by 2 (k - 1 - (i - j)) with i
    taken from np.nonzero, and at k = 32 a NumPy int64 shifted by 62 overflows where the Python int the model means does not."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def nonzero(x):
        return tuple(a.tolist() for a in np.nonzero(x))


_memo = {}


def _model(chars, lens, k, t=None):
    """M.correct of these rows, computed once per (rows, k, t) and left unchanged."""
    key = (chars.shape, hash(chars.tobytes()), hash(lens.tobytes()), k, t)
    if key not in _memo:
        keys, counts = M.count(chars, lens, k)
        M.np = _PlainIndices()
        try:
            want, changed, tt = M.correct(chars, lens, k, t)
        finally:
            M.np = np
        for a in (keys, counts, want, changed):
            a.setflags(write=False)
        _memo[key] = (keys, counts, want, changed, tt)
    return _memo[key]


def _check(batch, k, t=None, slots=None):
    """count_batch + correct_batch of `batch` against the model of its own rows."""
    from kbbq import kmer
    chars, lens = _rows(batch)
    keys, counts, want, want_changed, tt = _model(chars, lens, k, t)
    table = kmer.count_batch(batch, k=k, slots=slots)
    try:
        gk, gc = table.entries()
        assert np.array_equal(gk, keys) and np.array_equal(gc.astype(np.int64), counts)
        hist = kmer.kmer_histogram(table)
        assert np.array_equal(hist, M.histogram(counts))
        if t is None:
            assert kmer.solid_threshold(hist) == tt
        changed = kmer.correct_batch(table, batch, tt)
        assert batch.cseq is not None and batch.cseq.shape == batch.seq.shape and batch.cseq.data_ptr() != batch.seq.data_ptr()
        got = batch.chars('cseq')[:batch.n].cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(changed.cpu().numpy().astype(np.int64), want_changed)
        assert int(want_changed.sum()) > 0                      # the case corrects something
        assert np.array_equal(_rows(batch)[0], chars)            # the input plane is as it was
    finally:
        table.close()
    return keys, counts, want, tt


@pytest.fixture(scope='module')
def mixed():
    seq, meta = M.synth(11, genome_len=5000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
    return seq, meta


def _fixed(seed, S, genome_len=5000, paired=True, err=0.01):
    seq, meta = M.synth(seed, genome_len=genome_len, depth=30, err=err, len_lo=S, len_hi=S)[:2]
    n = seq.shape[0] & ~1
    seq, meta = seq[:n], meta[:n].copy()
    if paired:
        meta[1::2] |= SECOND
    return seq, meta


@pytest.mark.parametrize('k', [15, 31, 32])
def test_reads_nib_mixed_lengths(mixed, k):
    from kbbq import _device as dev
    seq, meta = mixed
    assert (seq == ord('N')).any()
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'reads_nib' and laid.cseq is None
    _check(laid, k)


def test_reads_nib_short_reads_and_chunk_edges():
    from kbbq import _device as dev
    rng = np.random.default_rng(3)
    genome = rng.integers(0, 4, 600)
    reads = []
    for L in (0, 5, 14, 15, 16, 17, 30, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81):
        for _ in range(40 if L else 1):
            s = int(rng.integers(0, 600 - L + 1))
            x = genome[s:s + L].copy()
            flip = rng.random(L) < 0.01
            x[flip] = (x[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
            reads.append(bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[x]))
    seq, meta = M.plane(reads)
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'reads_nib' and 0 in (_rows(laid)[1]).tolist()
    _check(laid, 15, t=3)
    _check(laid, 32, t=3)


@pytest.mark.parametrize('S,pitch', [(50, 112), (150, 304)])
@pytest.mark.parametrize('k', [21, 31])
def test_pairs_nib(S, pitch, k):
    from kbbq import _device as dev
    seq, meta = _fixed(20 + S, S, err=0.01 if S == 50 else 0.005)      # (the model walks every untrusted base in Python)
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'pairs_nib' and not laid.twins and laid.pitch == pitch and laid.n == seq.shape[0] // 2
    assert set(_rows(laid)[1].tolist()) == {2 * S + 1}
    _check(laid, k)


def test_twins_with_an_odd_number_of_reads():
    from kbbq import _device as dev
    seq, meta = _fixed(31, 100, paired=False)
    seq, meta = seq[:-1], meta[:-1]
    assert seq.shape[0] % 2 == 1
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'pairs_nib' and laid.twins and laid.n == (seq.shape[0] + 1) // 2
    _check(laid, 31)


def test_three_read_groups(mixed):
    from kbbq import _device as dev
    seq, meta = mixed
    rng = np.random.default_rng(5)
    meta = meta | (rng.integers(0, 3, meta.size).astype(np.uint32) << np.uint32(16))
    laid = dev.lay_out(_batch(seq, meta), 3)
    assert laid.layout_key() == 'reads_nib' and laid.seg is not None and laid.perm is not None
    perm = laid.perm.cpu().numpy()
    assert not np.array_equal(perm, np.arange(perm.size))
    keys, counts, _, _ = _check(laid, 21)
    k0, c0 = M.count(seq, meta, 21)                               # grouping only orders the rows
    assert np.array_equal(keys, k0) and np.array_equal(counts, c0)


def test_rows_of_more_than_256_chunks():
    from kbbq import _device as dev
    rng = np.random.default_rng(9)
    genome = rng.integers(0, 4, 4112)
    reads = []
    for L in (4112, 4112, 4112, 4111, 4100, 4097, 4112):
        x = genome[:L].copy()
        at = rng.choice(L, 4, replace=False)
        x[at] = (x[at] + rng.integers(1, 4, 4)) % 4
        reads.append(bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[x]))
    seq, meta = M.plane(reads)
    assert seq.shape[1] == 4112
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'reads_nib' and laid.pitch // 16 == 257
    _check(laid, 31, t=3)


def test_character_rows_through_the_same_calls(mixed):
    from kbbq import _device as dev
    seq, meta = mixed
    plain = _batch(seq, meta)
    assert plain.layout_key() == 'reads'
    _check(plain, 31)
    pseq, pmeta = _fixed(70, 50)
    laid = dev.lay_out(_batch(pseq, pmeta), 1, packed=False)
    assert laid.layout_key() == 'pairs' and laid.pitch == 112
    _check(laid, 21)


def test_one_table_from_character_and_nibble_rows(mixed):
    from kbbq import _device as dev
    from kbbq import kmer
    seq, meta = mixed
    h = seq.shape[0] // 2
    first, second = _batch(seq[:h], meta[:h]), dev.lay_out(_batch(seq[h:], meta[h:]), 1)
    assert (first.layout_key(), second.layout_key()) == ('reads', 'reads_nib')
    keys, counts = M.count(seq, meta, 31)
    table = kmer.count_batch(first, k=31, slots=1 << 20)
    kmer.count_batch(second, table=table)
    both = table.entries()
    table.close()
    assert np.array_equal(both[0], keys) and np.array_equal(both[1].astype(np.int64), counts)
    for whole in (_batch(seq, meta), dev.lay_out(_batch(seq, meta), 1)):
        t = kmer.count_batch(whole, k=31)
        alone = t.entries()
        t.close()
        assert np.array_equal(alone[0], both[0]) and np.array_equal(alone[1], both[1])


def test_prefilter_on_pairs_nib():
    from kbbq import _device as dev
    from kbbq import kmer
    k = 31
    seq, meta = _fixed(170, 150, err=0.005)                            # the rows of test_pairs_nib[.-150-304]: one model run
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'pairs_nib'
    chars, lens = _rows(laid)
    keys, counts, want, want_changed, t = _model(chars, lens, k)
    f = kmer.prefilter_batch(laid, k)
    assert f.words == kmer.filter_words(kmer.kmer_total(meta, k)) == 8192       # by the input's own sidecars: 1000 reads x 120 windows
    seen, twice = f.download()
    w, m = kmer.filter_index(keys, f.words)
    expect = np.zeros(f.words, dtype=np.uint64)
    np.bitwise_or.at(expect, w.astype(np.int64), m)
    assert np.array_equal(seen, expect)
    admitted = f.admitted
    f.release_seen()
    table = kmer.count_batch(laid, k=k, filter=f)
    plain = kmer.count_batch(laid, k=k)
    assert table.slots < plain.slots and 0 < admitted < int(counts.size)
    hist = kmer.kmer_histogram(table)
    assert np.array_equal(hist[2:], M.histogram(counts)[2:]) and np.array_equal(kmer.kmer_histogram(plain)[2:], hist[2:])
    assert kmer.solid_threshold(hist) == t
    changed = kmer.correct_batch(table, laid, t)
    filtered = laid.chars('cseq')[:laid.n].cpu().numpy()
    assert np.array_equal(filtered, want) and np.array_equal(changed.cpu().numpy().astype(np.int64), want_changed)
    kmer.correct_batch(plain, laid, t)
    assert np.array_equal(laid.chars('cseq')[:laid.n].cpu().numpy(), filtered)
    for x in (table, plain, f):
        x.close()


def test_a_table_of_too_few_slots(mixed):
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = mixed
    laid = dev.lay_out(_batch(seq, meta), 1)
    with pytest.raises(N.KmerTableFull, match='slots=1024'):
        kmer.count_batch(laid, k=31, slots=1024)
    keys, counts = M.count(seq, meta, 31)
    table = kmer.count_batch(laid, k=31)                           # the context goes on working
    gk, gc = table.entries()
    table.close()
    assert np.array_equal(gk, keys) and np.array_equal(gc.astype(np.int64), counts)


def test_bad_flags_and_planes_are_refused(mixed):
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = mixed
    laid = dev.lay_out(_batch(seq, meta), 1)
    lib, ctx = N.load(), dev.context()
    table = kmer.KmerTable(31, 1 << 16)
    args = (N.ptr(laid.seq), N.ptr(laid.meta), laid.n, laid.pitch)
    for flags in (8, N.ROWS_TWINS, N.ROWS_TWINS | N.ROWS_NIBBLES):
        with pytest.raises(ValueError, match='flags|TWINS'):
            N.check(lib.kbbq_kmer_count_rows_dev(ctx.handle, table.handle, *args, flags))
    with pytest.raises(ValueError, match='pitch'):
        N.check(lib.kbbq_kmer_count_rows_dev(ctx.handle, table.handle, N.ptr(laid.seq), N.ptr(laid.meta), laid.n, laid.pitch + 8,
                                             N.ROWS_NIBBLES))
    off = torch.empty(64, dtype=torch.uint8, device='cuda')[4:]
    with pytest.raises(ValueError, match='aligned'):
        N.check(lib.kbbq_kmer_correct_rows_dev(ctx.handle, table.handle, *args, N.ROWS_NIBBLES, 2, N.ptr(off), None))
    table.close()


_NATIVE = r'''
import sys
sys.path[:0] = [%(pkg)r, %(tests)r]
import numpy as np
import kmer_model as M
from kbbq import _device as dev, kmer
dev.use_native_memory()
seq, meta = M.synth(11, genome_len=5000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
qual = np.full(seq.shape, 63, dtype=np.uint8)
qual[np.arange(seq.shape[1])[None, :] >= meta.astype(np.int64)[:, None]] = 0
laid = dev.lay_out(dev.ReadBatch.from_host(seq, qual, meta), 1)
assert laid.layout_key() == 'reads_nib'
want, want_changed, t = M.correct(seq, meta, 31)
f = kmer.prefilter_batch(laid, 31)
f.release_seen()
table = kmer.count_batch(laid, k=31, filter=f)
assert kmer.solid_threshold(kmer.kmer_histogram(table)) == t
changed = kmer.correct_batch(table, laid, t)
assert np.array_equal(laid.chars('cseq')[:laid.n].cpu().numpy(), want)
assert np.array_equal(changed.cpu().numpy().astype(np.int64), want_changed)
assert 'torch' not in sys.modules
print('native ok', int(want_changed.sum()))
'''


def test_native_memory_backend():
    """The same calls on kbbq._hipmem tensors, in a process that never imports torch (the command line's back end)."""
    code = _NATIVE % dict(pkg=os.path.join(ROOT, 'kbbq-py_amd'), tests=os.path.join(ROOT, 'tests'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith('native ok')
