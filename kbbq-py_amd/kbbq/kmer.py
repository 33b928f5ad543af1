"""
K-mer counting and single-substitution error correction on the GPU (csrc/kbbq_kmer.h, include/kbbq_hip.h).

The reference has no corrector of its own: its tutorial (docs/tutorials/recalibration.rst, "Correcting Reads") runs an
external one and feeds its output to `kbbq recalibrate -f reads.fq reads.cor.fq`.  `kbbq correct` makes that file here:
every k-mer of every read is counted exactly in a device hash table, the first valley of the count histogram is the solid
threshold, and an untrusted base (no solid k-mer covers it) takes the one other base that makes the most covering k-mers
solid.  The rule, base by base, is in include/kbbq_hip.h; tests/kmer_model.py is a CPU model of it.

Planes are [n, pitch] uint8 seq planes with uint32 meta words (length in bits 0..15).  NumPy arrays go through the host-buffer
entry points (slab by slab through page-locked staging, any size); tensors on the GPU through the _dev ones.  There is no
CPU fallback.
"""
import ctypes
import sys

import numpy as np

from . import _native as N

HIST = 257
MIN_SLOTS = 1 << 10
SLOT_BYTES = 12
LOAD_FACTOR = 0.5


def _on_device(x):
    return hasattr(x, 'data_ptr') and getattr(x, 'is_cuda', False)


def _ctx():
    from . import _device as dev
    return dev.context()


def kmer_total(meta, k):
    """Number of k-mer windows (an upper bound on distinct k-mers) of reads with these meta words."""
    lens = np.asarray(meta, dtype=np.uint32).astype(np.int64) & 0xFFFF
    return int(np.maximum(lens - k + 1, 0).sum())


def default_slots(total, budget):
    """The table for `total` k-mer windows: a power of two at a load factor of at most 0.5, capped by `budget` bytes."""
    want = MIN_SLOTS
    while want * LOAD_FACTOR < total:
        want *= 2
    cap = MIN_SLOTS
    while cap * 2 * SLOT_BYTES <= budget:
        cap *= 2
    if cap * SLOT_BYTES > budget:
        raise ValueError('a k-mer table of slots=%d (%d bytes) does not fit the device budget of %d bytes (KBBQ_DEVICE_BUDGET)'
                         % (MIN_SLOTS, MIN_SLOTS * SLOT_BYTES, budget))
    return min(want, cap)


class KmerTable:
    """A device k-mer table (kbbq_kmer_table): `slots` (a power of two) 64-bit keys and 32-bit counts."""

    def __init__(self, k, slots, ctx=None):
        from . import _device as dev
        k, slots = int(k), int(slots)
        if not 8 <= k <= 32:
            raise ValueError('k must be in 8..32, got %d' % k)
        if slots < 16 or slots & (slots - 1):
            raise ValueError('slots must be a power of two >= 16, got %d' % slots)
        budget = dev.device_budget()
        need = int(N.load().kbbq_kmer_table_bytes(slots))
        if need > budget:
            raise ValueError('a k-mer table of slots=%d (%d bytes) does not fit the device budget of %d bytes '
                             '(KBBQ_DEVICE_BUDGET): give fewer slots' % (slots, need, budget))
        self.ctx = ctx or _ctx()
        self.k, self.slots = k, slots
        self._h = ctypes.c_void_p()
        N.check(N.load().kbbq_kmer_table_create_dev(self.ctx.handle, k, slots, ctypes.byref(self._h)))

    @property
    def handle(self):
        return self._h

    @property
    def nbytes(self):
        return int(N.load().kbbq_kmer_table_bytes(self.slots))

    def close(self):
        h = self.__dict__.pop('_h', None)
        if h:
            N.load().kbbq_kmer_table_free_dev(self.ctx.handle, h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def entries(self):
        """(keys uint64, counts uint32) of the occupied slots, sorted by key."""
        lib = N.load()
        dk, dc = ctypes.c_void_p(), ctypes.c_void_p()
        N.check(lib.kbbq_kmer_table_info(self._h, None, None, ctypes.byref(dk), ctypes.byref(dc)))
        keys = np.empty(self.slots, dtype=np.uint64)
        counts = np.empty(self.slots, dtype=np.uint32)
        N.check(lib.kbbq_dev_download(self.ctx.handle, N.ptr(keys), dk, keys.nbytes))
        N.check(lib.kbbq_dev_download(self.ctx.handle, N.ptr(counts), dc, counts.nbytes))
        used = keys != np.uint64(0xFFFFFFFFFFFFFFFF)
        keys, counts = keys[used], counts[used]
        order = np.argsort(keys, kind='stable')
        return keys[order], counts[order]


def _full(table, exc):
    return N.KmerTableFull('%s -- the table of slots=%d is too small for these reads: give more slots'
                           % (exc, table.slots))


def count_kmers(seq_plane, meta, k=31, slots=None, table=None):
    """Count every k-mer of the rows into `table` (a new one of `slots` slots when None; default: kmer_total at a load factor
    of at most 0.5, capped by the device budget) and return it.  Counting adds: several calls compose.  A table that fills
    raises KmerTableFull."""
    from . import _device as dev
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    if table is None:
        if slots is None:
            slots = default_slots(kmer_total(meta.cpu().numpy() if _on_device(meta) else meta, k), dev.device_budget())
        table = KmerTable(k, slots)
    lib = N.load()
    ctx = table.ctx
    try:
        if _on_device(seq_plane):
            N.check(lib.kbbq_kmer_count_dev(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch))
            ctx.status()
        else:
            seq_plane = np.ascontiguousarray(seq_plane, dtype=np.uint8)
            meta = np.ascontiguousarray(meta, dtype=np.uint32)
            N.check(lib.kbbq_kmer_count(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch))
    except N.KmerTableFull as exc:
        raise _full(table, exc) from None
    return table


def kmer_histogram(table):
    """h[c] = distinct k-mers with count c (c = 1..255), h[256] = those with count >= 256 (int64 [257], h[0] = 0)."""
    lib = N.load()
    ctx = table.ctx
    d = ctypes.c_void_p()
    N.check(lib.kbbq_dev_alloc(ctx.handle, HIST * 8, ctypes.byref(d)))
    try:
        N.check(lib.kbbq_kmer_histogram_dev(ctx.handle, table.handle, d))
        h = np.zeros(HIST, dtype=np.uint64)
        N.check(lib.kbbq_dev_download(ctx.handle, N.ptr(h), d, h.nbytes))
    finally:
        lib.kbbq_dev_free(ctx.handle, d)
    return h.astype(np.int64)


def solid_threshold(hist):
    """The first valley: the smallest c in 2..255 with h[c] <= h[c + 1].  ValueError when there is none."""
    h = np.asarray(hist)
    for c in range(2, 256):
        if h[c] <= h[c + 1]:
            return c
    raise ValueError('the k-mer count histogram has no valley in 2..255: give min_count')


def correct_with(table, seq_plane, meta, min_count):
    """(corrected plane, per-read changed-base counts uint32) of the rows against a counted table."""
    lib = N.load()
    ctx = table.ctx
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    if _on_device(seq_plane):
        out = seq_plane.new_empty(seq_plane.shape)
        changed = seq_plane.new_empty((max(n, 1),), dtype=__import__('torch').int32)
        N.check(lib.kbbq_kmer_correct_dev(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                          N.ptr(out), N.ptr(changed)))
        ctx.status()
        return out, changed[:n]
    seq_plane = np.ascontiguousarray(seq_plane, dtype=np.uint8)
    meta = np.ascontiguousarray(meta, dtype=np.uint32)
    out = np.empty_like(seq_plane)
    changed = np.zeros(max(n, 1), dtype=np.uint32)
    N.check(lib.kbbq_kmer_correct(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                  N.ptr(out), N.ptr(changed)))
    return out, changed[:n]


def correct_reads(seq_plane, meta, k=31, min_count=None, slots=None):
    """Count, pick the threshold (min_count, else the histogram's first valley) and correct.  Returns (corrected plane in
    the input's layout and kind, info) with info = {'k', 'min_count', 'hist', 'changed' (per read), 'slots', 'table_bytes'}."""
    table = count_kmers(seq_plane, meta, k=k, slots=slots)
    try:
        hist = kmer_histogram(table)
        t = int(min_count) if min_count is not None else solid_threshold(hist)
        if t < 1:
            raise ValueError('min_count must be >= 1, got %d' % t)
        out, changed = correct_with(table, seq_plane, meta, t)
        return out, dict(k=table.k, min_count=t, hist=hist, changed=changed, slots=table.slots, table_bytes=table.nbytes)
    finally:
        table.close()


def correct_fastq(path, out, k=31, min_count=None, slots=None):
    """Correct every read of a FASTQ file (plain or .gz) and write '@' + name, the corrected sequence, '+' and the qualities
    as read to `out` (a path, or a text stream).  Returns correct_reads' info."""
    from . import fastx
    fq = fastx.NativeFastq(path)
    try:
        n, S = fq.scan(None, False)[:2]
        pitch = fastx.pitch_for(S)
        seq, _, qual, meta = fq.fill(None, False, n, pitch)
        names = fq.names()
    finally:
        fq.close()
    fixed, info = correct_reads(seq, meta, k=k, min_count=min_count, slots=slots)
    text = fastx.format_fastq(names, fixed, qual, meta & 0xFFFF)
    if isinstance(out, str):
        with open(out, 'w', encoding='latin-1', newline='') as fh:
            fh.write(text)
    else:
        out.write(text)
        out.flush()
    info['reads'] = n
    return info


def main_correct(path, output=None, k=31, min_count=None, slots=None):
    """`kbbq correct`: the corrected FASTQ to `output` or stdout; the threshold and the changed bases to stderr."""
    info = correct_fastq(path, output if output else sys.stdout, k=k, min_count=min_count, slots=slots)
    sys.stderr.write('kbbq correct: k=%d min_count=%d reads=%d changed_bases=%d\n'
                     % (info['k'], info['min_count'], info['reads'], int(np.asarray(info['changed'], dtype=np.int64).sum())))
    return info
