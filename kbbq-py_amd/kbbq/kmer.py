"""
K-mer counting and single-substitution error correction on the GPU (csrc/kbbq_kmer.h, include/kbbq_hip.h).

The reference has no corrector of its own: its tutorial (docs/tutorials/recalibration.rst, "Correcting Reads") runs an
external one and feeds its output to `kbbq recalibrate -f reads.fq reads.cor.fq`.  `kbbq correct` makes that file here:
every k-mer of every read is counted exactly in a device hash table, the first valley of the count histogram is the solid
threshold, and an untrusted base (no solid k-mer covers it) takes the one other base that makes the most covering k-mers
solid.  The rule, base by base, is in include/kbbq_hip.h; tests/kmer_model.py is a CPU model of it.  With `fix_n` (`kbbq correct
--fix-n`) an N takes the letter that makes the most of the windows it alone breaks solid (the N rule of include/kbbq_hip.h;
tests/kmer_fixn_model.py); counting and the threshold do not change.  With `passes` = P > 1 (`kbbq correct --passes P`) the rule is applied to its own
output P times, row by row, against the same table (nothing is recounted): an error beside a read end, or beside another
error, is out of the rule's reach until its neighbour is corrected, and is within it afterwards (tests/kmer_passes_model.py).

Planes are [n, pitch] uint8 seq planes with uint32 meta words (length in bits 0..15).  NumPy arrays go through the host-buffer
entry points (slab by slab through page-locked staging, any size); tensors on the GPU through the _dev ones.  There is no
CPU fallback.  count_batch / prefilter_batch / correct_batch take _device.ReadBatch / PairBatch objects instead, in any layout
the recalibrate file path keeps reads in (4-bit planes, two reads to a row, rows grouped by read group), through the
kbbq_kmer_*_rows_dev calls: `kbbq recalibrate -c` corrects its reads where they lie (recalibrate.recalibrate_corrected).

Several ranks (one process per GPU under torch.distributed.run): every rank counts its own reads into a local table, sends each
key to the rank that owns it (owner(), a hash of the key that shares no bits with its home slot) and merges what it receives
into its owner table; the histogram is summed over ranks, every rank gathers the solid k-mers of all owner tables into a solid
table and corrects its own reads against it.  The rank files concatenated are the single-process output, byte for byte.

Prefilter (`prefilter=True`, one process): most distinct k-mers of real reads are errors seen once, and nothing after the count
looks at them.  A first pass over the reads marks every k-mer in a two-array bit filter (KmerFilter: `seen`, and `twice` for a
key whose bits were all in `seen` before); the count then skips every window that is not in `twice`.  The filter has no false
negatives, so every k-mer seen twice or more is counted exactly and the output is byte-identical; the table, sized from the
filter's `admitted` counter, is several times smaller.  h[1] of a filtered table counts only the once-seen keys the filter let
through, so min_count must be >= 2.

Partitions (`partitions=P`, `kbbq correct --partitions P|auto`, one process): the count split in time.  THE RULE:
part(key, P) = owner(key, P) (km_owner; kbbq_kmer_owner on the host).  For p = 0..P-1 the table -- 1/P the size -- is cleared
(except before the first round) and counts, over ALL rows of the input, exactly the windows whose canonical key has part == p
(kbbq_kmer_count*_part*).  A key lies in one partition, so its count there is its global count.  After each round
hist += kmer_histogram(table), and the pairs with count >= keep (select(table, 1, keep)) join the kept pairs on the device;
keep is min_count when given, else 2, the smallest value solid_threshold can return.  After the last round t is min_count or
solid_threshold(hist), the partition table is freed, ALL kept pairs are merged into a solid table of
default_slots(len(kept), budget) (those with keep <= count < t too: no decision reads them, and dropping them would cost a
pass over the pairs) and the unchanged correct / flag kernels run against it at min_count = t.  The summed histogram (with the
prefilter: h[2:]), the threshold, every base's decision and every figure printed are those of the one-table path; every round
hashes every window, which is what the smaller table costs.  In code: count_rounds is the rounds (`kbbq count` keeps their
pairs as they are), count_partitioned the rounds and the merge into the solid table.

The counting block (count_block) is the one place where the options above meet: the prefilter pass, `admitted`, the release
of `seen`, the number of rounds ('auto' included) within what the device budget leaves, the table's size, the count in one
round or in P, the histogram and the threshold -- or a k-mer set loaded in the count's place (load_set).  The commands that
decide bases (correct_reads; gatk.bqsr._kmer_tally for `bqsr --kmers` and `recalibrate -b --kmers`; benchmark.benchmark_kmers;
recalibrate.recalibrate_corrected) hand it a callback that runs one pass over all their rows and get (table, hist, t, info)
back; `kbbq count` shares its first half (count_plan) and count_rounds.

Quality gate (`kmer_min_qual=Q`, `--kmer-min-qual Q`; tests/kmer_gate_model.py).  THE RULE: a base is countable when it is A/C/G/T
and its quality -- the plane the command reads anyway -- is >= Q; a window is counted iff all k of its bases are countable.  One
kernel in front of the count (km_gate, kbbq_kmer_gate_rows_dev; gate_plane / gate_batch) writes a copy of the sequence plane with
'N' at every base below Q and returns the number of counted windows; the prefilter, the count, every partition round and a
rank's local count read that copy through the calls they always made, the filter and the default table are sized from the
counted windows, and the copy is freed when the count is over.  Nothing after the count knows the option: the histogram is the
gated table's, the threshold its first valley or min_count, and the correction, flag and passes calls run on the rows as read.
To count_block the gate is nothing but the caller's choice of rows and of `windows`: the callback reads the gated plane(s) in
the place of the sequence plane(s), and the counted windows stand where kmer_total or batch_windows would.
"""
import contextlib
import ctypes
import os
import sys

import numpy as np

from . import _bgzf
from . import _native as N

HIST = 257
MIN_SLOTS = 1 << 10
SLOT_BYTES = 12
LOAD_FACTOR = 0.5
MAX_BUCKETS = 1024                    # owners of one select (csrc/kbbq_kmer.h KM_MAX_BUCKETS)
OWNER_SALT = 0x9E3779B97F4A7C15
FILTER_SALT = 0xD6E8FEB86659FD93      # the prefilter's own salt (csrc/kbbq_kmer.h KM_FILTER_SALT)
FILTER_WORD_BYTES = 16                # a word of `seen` and one of `twice`


def _mix(x):
    """The table's 64-bit slot hash (km_hash) of uint64 arrays, wrapping as the device does."""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def owner(keys, world):
    """The rank (0..world-1) that owns each canonical key: the high 32 bits of the slot hash of key ^ OWNER_SALT, scaled to
    `world` (km_owner).  uint32 array of the keys' shape."""
    k = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over='ignore'):
        h = _mix(k ^ np.uint64(OWNER_SALT))
    return (((h >> np.uint64(32)) * np.uint64(int(world))) >> np.uint64(32)).astype(np.uint32)


def filter_index(keys, words):
    """(word index, mask) of each canonical key in a filter of `words` (a power of two) 64-bit words (km_filter_index):
    h = mix(key ^ FILTER_SALT), word = (h >> 24) & (words - 1), mask = the OR of 1 << ((h >> 6 j) & 63) for j = 0..3.
    uint64 arrays of the keys' shape."""
    words = int(words)
    if words < 1 or words & (words - 1):
        raise ValueError('words must be a power of two >= 1, got %d' % words)
    k = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over='ignore'):
        h = _mix(k ^ np.uint64(FILTER_SALT))
    mask = np.zeros(k.shape, dtype=np.uint64)
    for j in range(4):
        mask |= np.uint64(1) << ((h >> np.uint64(6 * j)) & np.uint64(63))
    return (h >> np.uint64(24)) & np.uint64(words - 1), mask


def filter_words(total, bits=4):
    """Words of each filter array for `total` k-mer windows: the smallest power of two with words * 64 >= bits * total."""
    total, bits = int(total), int(bits)
    if not 1 <= bits <= 64:
        raise ValueError('filter_bits must be in 1..64, got %d' % bits)
    words = 1
    while words * 64 < bits * total:
        words *= 2
    return words


MAX_PARTITIONS = 64                   # of one run (the kernels take up to MAX_BUCKETS)


def check_partitions(partitions):
    """`partitions` as an int in 1..MAX_PARTITIONS or the string 'auto', else ValueError: checked before any device call."""
    if isinstance(partitions, str):
        if partitions == 'auto':
            return partitions
    elif not isinstance(partitions, bool):
        try:
            if int(partitions) == partitions and 1 <= int(partitions) <= MAX_PARTITIONS:
                return int(partitions)
        except (TypeError, ValueError):
            pass
    raise ValueError("partitions must be an integer in 1..%d or 'auto', got %r" % (MAX_PARTITIONS, partitions))


def _wanted_slots(total):
    """The table for `total` keys at a load factor of at most 0.5, whatever the budget."""
    want = MIN_SLOTS
    while want * LOAD_FACTOR < total:
        want *= 2
    return want


def partition_windows(total, P):
    """What the table of one of P > 1 partitions is sized for: total / P and the slack of 9/8 that count_kmers_ranks gives owner
    tables (the partitions are as even as a hash makes them), rounded up."""
    return -(-int(total) * 9 // (8 * int(P)))


def partition_slots(total, P, budget):
    """The default table of one of P > 1 partitions of `total` windows (with the prefilter: admitted keys): half the budget is
    its, the other half is for the kept pairs and the solid table."""
    return default_slots(partition_windows(total, P), int(budget) // 2)


def partitions_for(total, budget):
    """The smallest P in 1..MAX_PARTITIONS whose default per-partition table fits half the budget uncapped (P = 1: `total` at a
    load factor of 0.5, without slack).  ValueError when MAX_PARTITIONS do not suffice."""
    total, half = int(total), int(budget) // 2
    for P in range(1, MAX_PARTITIONS + 1):
        if _wanted_slots(total if P == 1 else partition_windows(total, P)) * SLOT_BYTES <= half:
            return P
    raise ValueError('%d k-mer windows do not fit half the device budget of %d bytes (KBBQ_DEVICE_BUDGET) even in %d partitions '
                     '(a table of %d bytes each)' % (total, int(budget), MAX_PARTITIONS,
                                                     _wanted_slots(partition_windows(total, MAX_PARTITIONS)) * SLOT_BYTES))


def resolve_partitions(partitions, total, budget):
    """The number of rounds: `partitions` itself, or partitions_for(total, budget) for 'auto'."""
    return partitions_for(total, budget) if partitions == 'auto' else int(partitions)


def _check_partitions(partitions, launched=False):
    """check_partitions, and the refusal of anything but 1 in a process group (`launched`: under a launcher whose group does not
    exist yet): before any work on the GPU and, under ranks, before any collective."""
    partitions = check_partitions(partitions)
    if partitions != 1 and (launched or _ranks() is not None):
        raise ValueError('partitions do not run across ranks: the owner tables of a process group already split the k-mers W ways '
                         '(every rank holds the keys it owns), and a rank counts its own reads in rounds through a smaller table '
                         'with --local-slots; run without --partitions, or on one GPU')
    return partitions


def _partitions_kw(partitions):
    """The keyword for a callee: none at partitions = 1, whose calls are the ones they were before the option."""
    return dict(partitions=partitions) if partitions != 1 else {}


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

    def clear(self):
        """Empty every slot (asynchronous on the context's stream)."""
        N.check(N.load().kbbq_kmer_table_clear_dev(self.ctx.handle, self._h))

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


class KmerFilter:
    """A device k-mer filter (kbbq_kmer_filter): `words` (a power of two) 64-bit words of `seen` and of `twice`, and the
    `admitted` counter."""

    def __init__(self, words, ctx=None):
        from . import _device as dev
        words = int(words)
        if words < 1 or words & (words - 1):
            raise ValueError('words must be a power of two >= 1, got %d' % words)
        budget = dev.device_budget()
        need = int(N.load().kbbq_kmer_filter_bytes(words))
        if need > budget:
            raise ValueError('a k-mer filter of words=%d (%d bytes) does not fit the device budget of %d bytes '
                             '(KBBQ_DEVICE_BUDGET): give fewer filter bits' % (words, need, budget))
        self.ctx = ctx or _ctx()
        self.words = words
        self._seen = True
        self._h = ctypes.c_void_p()
        N.check(N.load().kbbq_kmer_filter_create_dev(self.ctx.handle, words, ctypes.byref(self._h)))

    @property
    def handle(self):
        return self._h

    @property
    def nbytes(self):
        """Device bytes held now: both arrays, or `twice` alone after release_seen."""
        full = int(N.load().kbbq_kmer_filter_bytes(self.words))
        return full if self._seen else full // 2

    @property
    def admitted(self):
        """OR-operations into `twice` that set a new bit so far: the keys the filtered count will insert, less the few whose
        mask other keys had completed (synchronises)."""
        v = ctypes.c_int64(0)
        N.check(N.load().kbbq_kmer_filter_admitted(self.ctx.handle, self._h, ctypes.byref(v)))
        return int(v.value)

    def close(self):
        h = self.__dict__.pop('_h', None)
        if h:
            N.load().kbbq_kmer_filter_free_dev(self.ctx.handle, h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        """Zero both arrays and the counter (asynchronous on the context's stream)."""
        N.check(N.load().kbbq_kmer_filter_clear_dev(self.ctx.handle, self._h))

    def release_seen(self):
        """Free `seen` once the last prefilter pass has been given: the filtered count reads `twice` alone."""
        N.check(N.load().kbbq_kmer_filter_release_seen_dev(self.ctx.handle, self._h))
        self._seen = False

    def download(self):
        """(seen, twice) as uint64 arrays of `words` words; seen is None after release_seen."""
        lib = N.load()
        ds, dt = ctypes.c_void_p(), ctypes.c_void_p()
        N.check(lib.kbbq_kmer_filter_info(self._h, None, ctypes.byref(ds), ctypes.byref(dt)))
        out = []
        for d in (ds, dt):
            if not d.value:
                out.append(None)
                continue
            a = np.empty(self.words, dtype=np.uint64)
            N.check(lib.kbbq_dev_download(self.ctx.handle, N.ptr(a), d, a.nbytes))
            out.append(a)
        return tuple(out)


def _host_meta(meta):
    return meta.cpu().numpy() if _on_device(meta) else meta


def prefilter_kmers(seq_plane, meta, k=31, filter=None, bits=4):
    """Pass every k-mer of the rows through `filter` (a new one of filter_words(kmer_total, bits) words when None) and return
    it.  Several calls compose; the filtered count comes after the last."""
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    k = int(k)
    if not 8 <= k <= 32:
        raise ValueError('k must be in 8..32, got %d' % k)
    if filter is None:
        filter = KmerFilter(filter_words(kmer_total(_host_meta(meta), k), bits))
    lib = N.load()
    ctx = filter.ctx
    if _on_device(seq_plane):
        N.check(lib.kbbq_kmer_prefilter_dev(ctx.handle, filter.handle, k, N.ptr(seq_plane), N.ptr(meta), n, pitch))
        ctx.status()
    else:
        seq_plane = np.ascontiguousarray(seq_plane, dtype=np.uint8)
        meta = np.ascontiguousarray(meta, dtype=np.uint32)
        N.check(lib.kbbq_kmer_prefilter(ctx.handle, filter.handle, k, N.ptr(seq_plane), N.ptr(meta), n, pitch))
    return filter


def _full(table, exc):
    return N.KmerTableFull('%s -- the table of slots=%d is too small for these reads: give more slots'
                           % (exc, table.slots))


def _check_part(parts, part):
    parts, part = int(parts), int(part)
    if not 1 <= parts <= MAX_BUCKETS:
        raise ValueError('parts must be in 1..%d, got %d' % (MAX_BUCKETS, parts))
    if not 0 <= part < parts:
        raise ValueError('part must be in 0..%d, got %d' % (parts - 1, part))
    return parts, part


# the count's entry points by (filter, parts > 1): for character planes (host buffers: the name without _dev) and for device batches
_COUNT = {(False, False): ('kbbq_kmer_count_dev', 'kbbq_kmer_count_rows_dev'),
          (True, False): ('kbbq_kmer_count_filtered_dev', 'kbbq_kmer_count_filtered_rows_dev'),
          (False, True): ('kbbq_kmer_count_part_dev', 'kbbq_kmer_count_rows_part_dev'),
          (True, True): ('kbbq_kmer_count_filtered_part_dev', 'kbbq_kmer_count_filtered_rows_part_dev')}


def _count_into(table, filter, rows, parts, part, batch=False, host=False):
    """One count call: `rows` (the plane, the sidecar and their sizes as the entry point takes them) into `table`, through the
    entry point that (device batch, host buffer, filter, parts > 1) name.  parts = 1 is the call without _part."""
    name = _COUNT[filter is not None, parts > 1][bool(batch)]
    call = getattr(N.load(), name[:-4] if host else name)
    args = (table.handle,) + ((filter.handle,) if filter is not None else ()) + tuple(rows) + ((parts, part) if parts > 1 else ())
    ctx = table.ctx
    try:
        N.check(call(ctx.handle, *args))
        if not host:
            ctx.status()
    except N.KmerTableFull as exc:
        raise _full(table, exc) from None
    return table


def count_kmers(seq_plane, meta, k=31, slots=None, table=None, filter=None, parts=1, part=0):
    """Count every k-mer of the rows into `table` (a new one of `slots` slots when None; default: kmer_total at a load factor
    of at most 0.5, capped by the device budget) and return it.  Counting adds: several calls compose.  A table that fills
    raises KmerTableFull.  With `filter` (a KmerFilter that has seen all the rows, prefilter_kmers) only the k-mers in its
    `twice` array are counted, and the default table is sized from filter.admitted instead of kmer_total.  With parts = P > 1
    only the windows whose key has owner(key, P) == part are counted (kbbq_kmer_count*_part*); parts = 1 is the call without."""
    from . import _device as dev
    parts, part = _check_part(parts, part)
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    if table is None:
        if slots is None:
            total = filter.admitted if filter is not None else kmer_total(_host_meta(meta), k)
            slots = default_slots(total, dev.device_budget())
        table = KmerTable(k, slots)
    host = not _on_device(seq_plane)
    if host:
        seq_plane = np.ascontiguousarray(seq_plane, dtype=np.uint8)
        meta = np.ascontiguousarray(meta, dtype=np.uint32)
    return _count_into(table, filter, (N.ptr(seq_plane), N.ptr(meta), n, pitch), parts, part, host=host)


def select(table, nbuckets=1, min_count=1):
    """The occupied slots with count >= min_count, sorted into `nbuckets` (1..MAX_BUCKETS) buckets by owner(key, nbuckets):
    (keys int64, counts int32, sizes) with keys / counts device tensors holding bucket 0's pairs, then bucket 1's, ... (any
    order inside a bucket; the keys' bits are uint64) and sizes an int64 NumPy array of the bucket sizes."""
    from . import _device as dev
    nbuckets, min_count = int(nbuckets), int(min_count)
    if not 1 <= nbuckets <= MAX_BUCKETS:
        raise ValueError('nbuckets must be in 1..%d, got %d' % (MAX_BUCKETS, nbuckets))
    lib = N.load()
    ctx = table.ctx
    sizes = np.zeros(nbuckets, dtype=np.int64)
    N.check(lib.kbbq_kmer_select_sizes_dev(ctx.handle, table.handle, nbuckets, min_count, N.ptr(sizes)))
    offsets = np.zeros(nbuckets, dtype=np.int64)
    np.cumsum(sizes[:-1], out=offsets[1:])
    total = int(sizes.sum())
    T = dev._torch()
    keys = T.empty(max(total, 1), dtype=T.int64, device='cuda')
    counts = T.empty(max(total, 1), dtype=T.int32, device='cuda')
    N.check(lib.kbbq_kmer_select_dev(ctx.handle, table.handle, nbuckets, min_count, N.ptr(offsets), N.ptr(keys), N.ptr(counts)))
    return keys[:total], counts[:total], sizes


def merge(table, keys, counts):
    """Add (key, count) pairs (device tensors of int64 / int32, as select returns) to `table`.  A table that fills raises
    KmerTableFull."""
    n = int(keys.shape[0])
    if int(counts.shape[0]) != n:
        raise ValueError('merge: %d keys but %d counts' % (n, int(counts.shape[0])))
    ctx = table.ctx
    try:
        N.check(N.load().kbbq_kmer_merge_dev(ctx.handle, table.handle, N.ptr(keys) if n else None, N.ptr(counts) if n else None, n))
        ctx.status()
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


def check_passes(passes):
    """`passes` as an int in 1..8 (KBBQ_E_ARG's range), else ValueError: checked before any device call and, under ranks, before
    any collective."""
    if isinstance(passes, bool) or int(passes) != passes or not 1 <= int(passes) <= N.KMER_MAX_PASSES:
        raise ValueError('passes must be an integer in 1..%d, got %r' % (N.KMER_MAX_PASSES, passes))
    return int(passes)


def correct_with(table, seq_plane, meta, min_count, fix_n=False, passes=1):
    """(corrected plane, per-read changed-base counts uint32) of the rows against a counted table.  fix_n: Ns are decided by the
    N rule (KBBQ_KMER_FIX_N) and a fixed N counts as a changed base.  passes: the rule applied to its own output that many
    times, a row at a time (kbbq_kmer_correct_passes*); the counts are then the bases that differ from the rows as read."""
    passes = check_passes(passes)
    lib = N.load()
    ctx = table.ctx
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    opts = N.KMER_FIX_N if fix_n else 0
    if _on_device(seq_plane):
        out = seq_plane.new_empty(seq_plane.shape)
        changed = seq_plane.new_empty((max(n, 1),), dtype=__import__('torch').int32)
        if passes > 1:
            N.check(lib.kbbq_kmer_correct_passes_dev(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch,
                                                     int(min_count), N.ptr(out), N.ptr(changed), opts, passes))
        else:
            N.check(lib.kbbq_kmer_correct_ex_dev(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                                 N.ptr(out), N.ptr(changed), opts))
        ctx.status()
        return out, changed[:n]
    seq_plane = np.ascontiguousarray(seq_plane, dtype=np.uint8)
    meta = np.ascontiguousarray(meta, dtype=np.uint32)
    out = np.empty_like(seq_plane)
    changed = np.zeros(max(n, 1), dtype=np.uint32)
    if passes > 1:
        N.check(lib.kbbq_kmer_correct_passes(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                             N.ptr(out), N.ptr(changed), opts, passes))
    else:
        N.check(lib.kbbq_kmer_correct_ex(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                         N.ptr(out), N.ptr(changed), opts))
    return out, changed[:n]


def flag_errors(table, seq_plane, meta, min_count, unresolved=False, passes=1):
    """(flag plane uint8 [n, pitch], per-read flagged-base counts int32) of device rows against a counted table
    (kbbq_kmer_flag_dev): 1 exactly where correct_with would write another letter, 0 everywhere else, padding included.
    The plane is the one plane of flags the aligned tally reads (bit 0 error; gatk.bqsr.bam_to_kmer_covariates).  Device
    tensors in, device tensors out; there is no host-buffer form.
    unresolved: (flag plane, flagged-base counts, unresolved-base counts int32) of kbbq_kmer_flag_ex_dev with
    KBBQ_KMER_FLAG_UNRESOLVED -- an untrusted A/C/G/T base for which no substitution wins (a tie, or none makes a solid k-mer)
    is 2 in the plane, the tally's skip bit; every other byte is what it is without the option.
    passes > 1 (kbbq_kmer_flag_passes_dev): 1 where `passes` passes of the correction end on another letter than the read's, 2
    (with `unresolved`) where the base is unchanged and the last evaluation of its row left it unresolved."""
    from . import _device as dev
    passes = check_passes(passes)
    if not _on_device(seq_plane):
        raise TypeError('flag_errors takes device planes (correct_with takes host buffers too)')
    T = dev._torch()
    ctx = table.ctx
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    flags = T.empty((max(n, 1), pitch), dtype=T.uint8, device=seq_plane.device)
    changed = T.empty((max(n, 1),), dtype=T.int32, device=seq_plane.device)
    if passes > 1:
        skipped = T.empty((max(n, 1),), dtype=T.int32, device=seq_plane.device)
        N.check(N.load().kbbq_kmer_flag_passes_dev(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                                   N.ptr(flags), N.ptr(changed), N.ptr(skipped),
                                                   N.KMER_FLAG_UNRESOLVED if unresolved else 0, passes))
        ctx.status()
        return (flags[:n], changed[:n], skipped[:n]) if unresolved else (flags[:n], changed[:n])
    if unresolved:
        skipped = T.empty((max(n, 1),), dtype=T.int32, device=seq_plane.device)
        N.check(N.load().kbbq_kmer_flag_ex_dev(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                               N.ptr(flags), N.ptr(changed), N.ptr(skipped), N.KMER_FLAG_UNRESOLVED))
        ctx.status()
        return flags[:n], changed[:n], skipped[:n]
    N.check(N.load().kbbq_kmer_flag_dev(ctx.handle, table.handle, N.ptr(seq_plane), N.ptr(meta), n, pitch, int(min_count),
                                        N.ptr(flags), N.ptr(changed)))
    ctx.status()
    return flags[:n], changed[:n]


# ---- device batches in the recalibrate path's layouts ------------------------------------------------------------------------

def batch_windows(batch, k):
    """K-mer windows of a _device.ReadBatch / PairBatch of any layout (what sizes its table and filter).  A row of two reads
    is counted as its two reads of S bases, not as the one row of 2S + 1 its sidecar describes."""
    from . import _device as dev
    if isinstance(batch, dev.PairBatch):
        # an upper bound by one read for twin rows of an odd number of reads (the last row's second half is padding)
        return 2 * batch.n * max(batch.S - int(k) + 1, 0)
    if batch.n == 0:
        return 0
    return kmer_total(batch.meta[:batch.n].cpu().numpy().view(np.uint32), k)


def _batch_rows(batch):
    """(seq, meta, rows, pitch, KBBQ_ROWS_* flags) of a device batch for the kbbq_kmer_*_rows_dev calls."""
    from . import _device as dev
    return N.ptr(batch.seq), N.ptr(batch.meta), int(batch.n), int(batch.pitch), dev._row_flags(batch)


# ---- the quality gate ---------------------------------------------------------------------------------------------------------

MAX_MIN_QUAL = 93                     # the top of the FASTQ scale: '~' - 33


def check_kmer_min_qual(min_qual, have_qual=True):
    """`min_qual` as an int in 1..MAX_MIN_QUAL, or None when it is None (no gate), else ValueError: checked before any device
    call and, under ranks, before any collective.  have_qual: False when the caller has no qualities to gate by."""
    if min_qual is None:
        return None
    ok = False
    if not isinstance(min_qual, (bool, str, bytes)):
        try:
            ok = int(min_qual) == min_qual and 1 <= int(min_qual) <= MAX_MIN_QUAL
        except (TypeError, ValueError):
            ok = False
    if not ok:
        raise ValueError('kmer_min_qual must be an integer in 1..%d, got %r' % (MAX_MIN_QUAL, min_qual))
    if not have_qual:
        raise ValueError('kmer_min_qual=%d needs the qualities of the reads: there is no quality plane to gate by' % int(min_qual))
    return int(min_qual)


def _gate_rows(ctx, seq, qual, meta, n, pitch, flags, k, byte_min, out, windows):
    N.check(N.load().kbbq_kmer_gate_rows_dev(ctx.handle, seq, qual, meta, n, pitch, flags, int(k), int(byte_min), out, windows))
    ctx.status()


def _to_device(T, a, dtype=None):
    """A host array as a device tensor of the backend in use; a device tensor as it is."""
    if _on_device(a):
        return a
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = T.empty(a.shape if a.size else (1,) + a.shape[1:], dtype=getattr(T, a.dtype.name), device='cuda')
    if a.size:
        t[:a.shape[0]].copy_(T.from_numpy(a))
    return t


def gate_plane(seq_plane, qual_plane, meta, k, min_qual, qual_offset=33, windows=None):
    """The quality gate of character rows, one read a row (kbbq_kmer_gate_rows_dev, flags 0): (gated plane, counted windows).
    The gated plane is a device copy of seq_plane with 'N' wherever the byte of qual_plane is < min_qual + qual_offset
    (qual_offset: 33 for character qualities, 0 for a plane of raw Phred values), so every count and prefilter call on it --
    with the same meta -- sees exactly the windows whose k bases are all A/C/G/T of quality >= min_qual; counted windows is
    their number.  Host arrays are uploaded (there is no host-buffer form); seq_plane itself is never written.
    windows: a zeroed one-word int64 device tensor to add to instead of a new one (several planes of one input); the return is
    then its value after this plane."""
    from . import _device as dev
    min_qual = check_kmer_min_qual(min_qual, qual_plane is not None)
    T = dev._torch()
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    seq, qual, meta = _to_device(T, seq_plane, np.uint8), _to_device(T, qual_plane, np.uint8), _to_device(T, meta, np.uint32)
    out = T.empty((max(n, 1), pitch), dtype=T.uint8, device='cuda')
    if windows is None:
        windows = T.zeros(1, dtype=T.int64, device='cuda')
    _gate_rows(_ctx(), N.ptr(seq), N.ptr(qual), N.ptr(meta), n, pitch, 0, k, min_qual + int(qual_offset), N.ptr(out), N.ptr(windows))
    return out[:n], int(windows.cpu().numpy()[0])


def count_windows(seq_plane, meta, k, windows=None):
    """The number of k-mer windows of character rows that a count inserts: those whose k bases are all A/C/G/T inside the read
    (kmer_total counts the broken ones too).  It is kbbq_kmer_gate_rows_dev with the sequence plane as its own quality plane and
    the threshold 1, which every character passes; the copy it writes is dropped.  windows: as gate_plane's."""
    from . import _device as dev
    T = dev._torch()
    n, pitch = int(seq_plane.shape[0]), int(seq_plane.shape[1])
    seq, meta = _to_device(T, seq_plane, np.uint8), _to_device(T, meta, np.uint32)
    out = T.empty((max(n, 1), pitch), dtype=T.uint8, device='cuda')
    if windows is None:
        windows = T.zeros(1, dtype=T.int64, device='cuda')
    _gate_rows(_ctx(), N.ptr(seq), N.ptr(seq), N.ptr(meta), n, pitch, 0, k, 1, N.ptr(out), N.ptr(windows))
    return int(windows.cpu().numpy()[0])


def gate_batch(batch, k, min_qual, windows=None, qual=None):
    """gate_plane for the rows of a device batch in whatever layout it has: (gated plane in the layout of batch.seq, counted
    windows).  The qualities are batch.qual (characters, offset 33) unless `qual` names another plane of that geometry.
    prefilter_batch / count_batch read the gated plane through their `plane` argument; batch.seq is not written."""
    from . import _device as dev
    min_qual = check_kmer_min_qual(min_qual)
    T = dev._torch()
    out = T.empty_like(batch.seq)
    if windows is None:
        windows = T.zeros(1, dtype=T.int64, device='cuda')
    seq, meta, n, pitch, flags = _batch_rows(batch)
    _gate_rows(_ctx(), seq, N.ptr(batch.qual if qual is None else qual), meta, n, pitch, flags, k, min_qual + 33, N.ptr(out),
               N.ptr(windows))
    return out, int(windows.cpu().numpy()[0])


def min_qual_field(info):
    """` kmer_min_qual=Q counted_windows=N` of a command's stderr line when its count was gated, else nothing."""
    if info.get('kmer_min_qual') is None:
        return ''
    return ' kmer_min_qual=%d counted_windows=%d' % (info['kmer_min_qual'], info['counted_windows'])


def _min_qual_kw(kmer_min_qual, **more):
    """The keywords for a callee: none without the gate, whose calls are the ones they were before the option."""
    return dict(kmer_min_qual=kmer_min_qual, **more) if kmer_min_qual is not None else {}


def prefilter_batch(batch, k, filter=None, bits=4, plane=None):
    """prefilter_kmers for the rows of a device batch in whatever layout it has (layout_key() reads / reads_nib / pairs /
    pairs_nib, twins, rows grouped by read group): the same `seen` words as the character planes of the same reads give.
    plane: a plane of batch.seq's layout to read in its place (gate_batch's)."""
    k = int(k)
    if not 8 <= k <= 32:
        raise ValueError('k must be in 8..32, got %d' % k)
    if filter is None:
        filter = KmerFilter(filter_words(batch_windows(batch, k), bits))
    seq, meta, n, pitch, flags = _batch_rows(batch)
    if plane is not None:
        seq = N.ptr(plane)
    ctx = filter.ctx
    N.check(N.load().kbbq_kmer_prefilter_rows_dev(ctx.handle, filter.handle, k, seq, meta, n, pitch, flags))
    ctx.status()
    return filter


def count_batch(batch, k=31, table=None, slots=None, filter=None, parts=1, part=0, plane=None):
    """count_kmers for the rows of a device batch in whatever layout it has: the reads are counted where they lie.  Keys and
    counts are those of the character planes of the same reads, so batches of different layouts compose in one table.
    parts, part: as count_kmers' (kbbq_kmer_count*_rows_part_dev).  plane: a plane of batch.seq's layout to read in its place
    (gate_batch's; the default table is still sized from the batch's windows: give `slots`)."""
    from . import _device as dev
    parts, part = _check_part(parts, part)
    if table is None:
        if slots is None:
            slots = default_slots(filter.admitted if filter is not None else batch_windows(batch, k), dev.device_budget())
        table = KmerTable(k, slots)
    seq, meta, n, pitch, flags = _batch_rows(batch)
    if plane is not None:
        seq = N.ptr(plane)
    return _count_into(table, filter, (seq, meta, n, pitch, flags), parts, part, batch=True)


def correct_batch(table, batch, min_count, fix_n=False, passes=1, skip_unresolved=False):
    """Correct the rows of a device batch against a counted table into batch.cseq (allocated here when the batch was made
    without one) in the batch's own layout: K1 takes it as it is.  Returns `changed`, the changed bases per ROW as an int32
    device array (a row of two reads counts both).  fix_n: the N rule, in every layout (a fixed N of a 4-bit plane is its
    letter's code; the separator of a row of two reads is no N).  passes: as correct_with's, in every layout.
    skip_unresolved (kbbq_kmer_correct_rows_skip_dev): the batch also gets batch.tally_qual, its quality plane with byte 0 at
    every unresolved base (untrusted, and no substitution wins) -- K1 with that plane in the place of batch.qual tallies those
    bases neither as errors nor as observations -- and the return is (changed, unresolved), both per row; batch.cseq and
    `changed` are what they are without."""
    from . import _device as dev
    passes = check_passes(passes)
    T = dev._torch()
    if batch.cseq is None:
        batch.cseq = T.empty_like(batch.seq)
    seq, meta, n, pitch, flags = _batch_rows(batch)
    changed = T.empty((max(n, 1),), dtype=T.int32, device=batch.seq.device)
    ctx = table.ctx
    if skip_unresolved:
        batch.tally_qual = T.empty_like(batch.qual)
        unresolved = T.empty((max(n, 1),), dtype=T.int32, device=batch.seq.device)
        N.check(N.load().kbbq_kmer_correct_rows_skip_dev(ctx.handle, table.handle, seq, meta, n, pitch, flags, int(min_count),
                                                         N.ptr(batch.cseq), N.ptr(changed), N.KMER_FIX_N if fix_n else 0, passes,
                                                         N.ptr(batch.qual), N.ptr(batch.tally_qual), N.ptr(unresolved)))
        ctx.status()
        return changed[:n], unresolved[:n]
    if passes > 1:
        N.check(N.load().kbbq_kmer_correct_rows_passes_dev(ctx.handle, table.handle, seq, meta, n, pitch, flags, int(min_count),
                                                           N.ptr(batch.cseq), N.ptr(changed), N.KMER_FIX_N if fix_n else 0, passes))
    else:
        N.check(N.load().kbbq_kmer_correct_rows_ex_dev(ctx.handle, table.handle, seq, meta, n, pitch, flags, int(min_count),
                                                       N.ptr(batch.cseq), N.ptr(changed), N.KMER_FIX_N if fix_n else 0))
    ctx.status()
    return changed[:n]


def partitions_field(info):
    """` partitions=P` of a command's stderr line when its count took P > 1 rounds, else nothing."""
    return ' partitions=%d' % info['partitions'] if info.get('partitions', 1) > 1 else ''


def _passes_kw(passes):
    """The keyword for a callee: none at passes = 1, whose calls are the ones they were before the option."""
    return dict(passes=passes) if passes != 1 else {}


def _check_prefilter(min_count, filter_bits):
    """The prefilter's rules, checked before any work on the GPU and, under ranks, before any collective."""
    if min_count is not None and int(min_count) < 2:
        raise ValueError('min_count must be >= 2 with the prefilter, got %d: k-mers seen once are not counted' % int(min_count))
    if not 1 <= int(filter_bits) <= 64:
        raise ValueError('filter_bits must be in 1..64, got %d' % int(filter_bits))
    if _ranks() is not None:
        raise ValueError('the prefilter does not run across ranks yet: a k-mer seen once on each of two ranks is not seen '
                         'once, so the filter belongs at the rank that owns the key; run on one GPU, or without the prefilter')


def count_rounds(count_round, k, P, slots, keep):
    """The rounds of the module docstring's "Partitions" through one table of `slots` slots: for p = 0..P-1 the table is cleared
    (except before the first round), count_round(table, p) counts partition p of P of the WHOLE input into it, its histogram is
    added to `hist` and its pairs with count >= keep join `kept` on the device.  P = 1 is one count that clears nothing.
    Returns (hist, kept, info): the summed histogram, the list of (keys, counts) device pairs of the rounds that kept any, and
    info = {'partitions', 'slots', 'table_bytes'}.  The table is closed here; count_round's KmerTableFull passes through."""
    P = int(P)
    hist = np.zeros(HIST, dtype=np.int64)
    kept = []                                # (keys, counts) of every round, on the device
    table = KmerTable(k, slots)
    try:
        info = dict(partitions=P, slots=table.slots, table_bytes=table.nbytes)
        for p in range(P):
            if p:
                table.clear()
            count_round(table, p)
            hist += kmer_histogram(table)
            keys, counts, _ = select(table, 1, keep)
            if int(keys.shape[0]):
                kept.append((keys, counts))
            del keys, counts
    finally:
        table.close()
    return hist, kept, info


def count_partitioned(count_round, k, P, slots, min_count, budget):
    """The rule of the module docstring's "Partitions", which count_block runs for every command: count_rounds, then the merge
    of all kept pairs into the solid table.  count_round(table, p) counts partition p of P of the WHOLE input (a plane, or every
    band's rows) into `table`; `slots` is the per-partition table, `budget` what the solid table may take.  Returns (solid table, hist, t, info): the table the correct / flag kernels read at
    min_count = t, the histogram summed over the rounds, and info = {'partitions', 'slots', 'table_bytes' (the per-partition
    table), 'kept_pairs', 'solid_slots'}.  A round whose table fills raises count_round's KmerTableFull."""
    if min_count is not None and int(min_count) < 1:
        raise ValueError('min_count must be >= 1, got %d' % int(min_count))
    hist, kept, info = count_rounds(count_round, k, P, slots, int(min_count) if min_count is not None else 2)
    t = int(min_count) if min_count is not None else solid_threshold(hist)
    npairs = sum(int(keys.shape[0]) for keys, _ in kept)
    solid = KmerTable(k, default_slots(npairs, budget))
    try:
        for keys, counts in kept:
            merge(solid, keys, counts)
    except BaseException:
        solid.close()
        raise
    info.update(kept_pairs=npairs, solid_slots=solid.slots)
    return solid, hist, t, info


# ---- k-mer sets (kbbq/kmerset.py) ---------------------------------------------------------------------------------------------

PAIR_REASONS = {1: 'its key is not above the key before it (unsorted, or a duplicate)', 2: 'its key is not below 4^k',
                3: 'its key is not canonical (it is above its reverse complement)', 4: 'its count is below keep'}


def sort_pairs(kept, k):
    """All (keys int64, counts int32) device pairs of the list `kept` (as select returns them; the list is emptied, so each
    piece is released once it is copied) as ONE pair of device tensors sorted ascending by UNSIGNED key
    (kbbq_kmer_sort_pairs_dev over the 2k key bits: a k = 32 key with bit 63 set sorts last, not first).  At the peak the
    device holds the pieces' 12 n bytes, then the sorted copy's 12 n beside them and the sort's temporary."""
    from . import _device as dev
    T = dev._torch()
    lib = N.load()
    ctx = _ctx()
    n = sum(int(keys.shape[0]) for keys, _ in kept)
    if len(kept) == 1:
        keys, counts = kept.pop()
    else:
        keys = T.empty(max(n, 1), dtype=T.int64, device='cuda')
        counts = T.empty(max(n, 1), dtype=T.int32, device='cuda')
        at = 0
        while kept:
            kk, cc = kept.pop(0)
            m = int(kk.shape[0])
            if m:
                keys[at:at + m].copy_(kk)
                counts[at:at + m].copy_(cc)
            at += m
            del kk, cc
    if n == 0:
        return keys[:0], counts[:0]
    out_keys = T.empty(n, dtype=T.int64, device='cuda')
    out_counts = T.empty(n, dtype=T.int32, device='cuda')
    need = ctypes.c_size_t(0)
    N.check(lib.kbbq_kmer_sort_pairs_bytes(ctx.handle, n, ctypes.byref(need)))
    temp = T.empty(max(int(need.value), 16), dtype=T.uint8, device='cuda')
    N.check(lib.kbbq_kmer_sort_pairs_dev(ctx.handle, int(k), N.ptr(keys), N.ptr(counts), N.ptr(out_keys), N.ptr(out_counts), n,
                                         N.ptr(temp), int(need.value)))
    ctx.sync()
    return out_keys, out_counts


def check_pairs(keys, counts, k, keep, first=0, prev=None, sums=None):
    """kbbq_kmer_check_pairs_dev on one slab of device pairs: (sums, bad).  sums: a uint64 [2] NumPy array the slab's key and
    count sums (mod 2^64) are ADDED to (a new one when None); bad: None, or (global pair index, reason text) of the lowest pair
    that is not above the key before it (`prev` for the slab's first, when given), not below 4^k, not canonical or below keep."""
    n = int(keys.shape[0])
    if sums is None:
        sums = np.zeros(2, dtype=np.uint64)
    if n == 0:
        return sums, None
    ctx = _ctx()
    index, why = ctypes.c_int64(-1), ctypes.c_int(0)
    N.check(N.load().kbbq_kmer_check_pairs_dev(ctx.handle, N.ptr(keys), N.ptr(counts), n, int(k), int(keep), int(first),
                                               0 if prev is None else 1, 0 if prev is None else int(prev), N.ptr(sums),
                                               ctypes.byref(index), ctypes.byref(why)))
    return sums, (None if index.value < 0 else (int(index.value), PAIR_REASONS.get(int(why.value), 'reason %d' % why.value)))


COUNTING_OPTIONS = ('prefilter', 'filter_bits', 'partitions', 'kmer_min_qual', 'local_slots')


def check_kmers_from(kmers_from, prefilter=False, filter_bits=4, partitions=1, kmer_min_qual=None, local_slots=None):
    """The one refusal of every call that takes kmers_from: a loaded set takes no counting options.  Returns the path (None:
    nothing is loaded and nothing is checked).  No device, no collective."""
    if kmers_from is None:
        return None
    given = [name for name, v, default in (('prefilter', bool(prefilter), False), ('filter_bits', filter_bits, 4),
                                           ('partitions', partitions, 1), ('kmer_min_qual', kmer_min_qual, None),
                                           ('local_slots', local_slots, None)) if v is not None and v != default]
    if given:
        raise ValueError('%s: not with kmers_from: these are counting options, and the k-mers come counted from %s'
                         % (', '.join(given), kmers_from))
    return os.fspath(kmers_from)


def kmers_from_field(info):
    """` kmers_from=1 loaded_kmers=N` at the very end of a command's stderr line when its k-mers were loaded, else nothing."""
    return ' kmers_from=1 loaded_kmers=%d' % info['loaded_kmers'] if info.get('kmers_from') else ''


def summary_line(command, info, options, bases='changed_bases'):
    """The one stderr line of a k-mer command, `kbbq COMMAND: k=.. min_count=.. reads=.. ..\\n`, from the `info` its library call
    returned and the k-mer keywords `options` it was made with: ` excluded_reads=N` with exclude_flags, then info[bases]
    (changed_bases, or flagged_bases of the commands that only flag), ` skipped_bases=N` with skip_unresolved, ` fix_n=1`,
    ` passes=P` above one pass, partitions_field, min_qual_field, with the prefilter the admitted k-mers and the table's slots,
    and kmers_from_field at the very end."""
    return ('kbbq %s: k=%d min_count=%d reads=%d%s %s=%d%s%s%s%s%s%s%s\n'
            % (command, info['k'], info['min_count'], info['reads'],
               ' excluded_reads=%d' % info['excluded_reads'] if options.get('exclude_flags') else '', bases, info[bases],
               ' skipped_bases=%d' % info['skipped_bases'] if options.get('skip_unresolved') else '',
               ' fix_n=1' if options.get('fix_n') else '', ' passes=%d' % options['passes'] if options.get('passes', 1) > 1 else '',
               partitions_field(info), min_qual_field(info),
               ' prefilter=1 admitted=%d slots=%d' % (info['admitted'], info['slots']) if options.get('prefilter') else '',
               kmers_from_field(info)))


def _kmers_from_kw(kmers_from):
    """The keyword for a callee: none without a set, whose calls are the ones they were before the option."""
    return dict(kmers_from=kmers_from) if kmers_from is not None else {}


def set_k(kmers_from, k=None):
    """The k of a k-mer set (a path, whose header is read, or a kmerset.KmerSet); an explicit `k` that differs is a ValueError
    naming both.  No device."""
    from . import kmerset
    s = kmers_from if isinstance(kmers_from, kmerset.KmerSet) else kmerset.open_set(kmers_from)
    if k is not None and int(k) != s.k:
        raise ValueError('k = %d was asked for, but the k-mer set %s was counted with k = %d' % (int(k), s.path, s.k))
    return s.k


def load_set(path, min_count=None, slots=None, k=None, budget=None, slab=None):
    """A k-mer set file (kbbq/kmerset.py) as the tuple every counting block ends with: (table, hist, t, info).  k is the file's
    (an explicit `k` that differs is a ValueError naming both); t is min_count (below the file's keep: ValueError naming both)
    or the first valley of the file's histogram at or above keep (kmerset.set_threshold; none: solid_threshold's ValueError).
    ALL n pairs are loaded, those with keep <= count < t too, as count_partitioned merges all it kept: no decision reads them,
    and leaving them out would cost a compaction pass per slab.  The table has `slots` slots, else default_slots(n, budget)
    (budget: the device budget); one that is too small raises KmerTableFull.  The file is read slab by slab (`slab` pairs,
    default kmerset.slab_pairs(): KBBQ_STAGE_MB) into one page-locked buffer, uploaded, CHECKED ON THE DEVICE
    (check_pairs; the last key of a slab is handed to the next) and merged (kbbq_kmer_merge_dev): host memory does not grow with
    n.  A pair that fails raises ValueError('k-mer set PATH: pair I: ...'), sums that differ from the header's
    ValueError('... checksum ...'); either way the table is closed and no kernel has read it.
    info: k, keep, min_qual, reads, windows, kmers_from (the path), loaded_kmers, slots, table_bytes."""
    from . import _device as dev
    from . import kmerset
    s = kmerset.open_set(path)
    set_k(s, k)
    if min_count is not None:
        if int(min_count) < s.keep:
            raise ValueError('min_count = %d is below keep = %d of the k-mer set %s: the k-mers seen fewer than %d times are not '
                             'in it' % (int(min_count), s.keep, s.path, s.keep))
        t = int(min_count)
    else:
        t = kmerset.set_threshold(s.hist, s.keep)
    T = dev._torch()
    n = s.n
    pairs = max(min(int(slab) if slab else kmerset.slab_pairs(), max(n, 1)), 1)
    if slots is None:
        slots = default_slots(n, dev.device_budget() if budget is None else budget)
    table = KmerTable(s.k, slots)
    try:
        if n:
            host = dev.pinned('kmerset', 0, pairs * 12)
            d_keys = T.empty(pairs, dtype=T.int64, device='cuda')
            d_counts = T.empty(pairs, dtype=T.int32, device='cuda')
            sums = np.zeros(2, dtype=np.uint64)
            prev = None
            with open(s.path, 'rb') as fh:
                for lo in range(0, n, pairs):
                    m = min(pairs, n - lo)
                    h_keys, h_counts = host[:8 * m].view(T.int64), host[8 * pairs:8 * pairs + 4 * m].view(T.int32)
                    for at, h in ((s.keys_offset + 8 * lo, h_keys), (s.counts_offset + 4 * lo, h_counts)):
                        fh.seek(at)
                        raw = h.numpy().view(np.uint8)
                        if fh.readinto(memoryview(raw)) != raw.nbytes:
                            raise ValueError('k-mer set %s: the file ends inside its pairs' % s.path)
                    last = int(h_keys.numpy().view(np.uint64)[m - 1])
                    d_keys[:m].copy_(h_keys)
                    d_counts[:m].copy_(h_counts)
                    _, bad = check_pairs(d_keys[:m], d_counts[:m], s.k, s.keep, first=lo, prev=prev, sums=sums)
                    if bad is not None:
                        raise ValueError('k-mer set %s: pair %d: %s' % (s.path, bad[0], bad[1]))
                    merge(table, d_keys[:m], d_counts[:m])
                    prev = last
            del d_keys, d_counts, host
            dev.release_pinned('kmerset')
            if (int(sums[0]), int(sums[1])) != (s.key_sum, s.count_sum):
                raise ValueError('k-mer set %s: checksum: the pairs sum to (%d, %d), the header says (%d, %d)'
                                 % (s.path, int(sums[0]), int(sums[1]), s.key_sum, s.count_sum))
        elif (s.key_sum, s.count_sum) != (0, 0):
            raise ValueError('k-mer set %s: checksum: no pairs, but the header says (%d, %d)' % (s.path, s.key_sum, s.count_sum))
    except BaseException:
        table.close()
        raise
    info = dict(k=s.k, keep=s.keep, min_qual=s.min_qual, reads=s.reads, windows=s.windows, kmers_from=s.path, loaded_kmers=n,
                slots=table.slots, table_bytes=table.nbytes)
    return table, s.hist.copy(), t, info


def _untimed(name, sync=True):
    """stage() of a caller that times nothing."""
    return contextlib.nullcontext()


def count_plan(read, windows, slots=None, prefilter=False, filter_bits=4, partitions=1, room=None, stage=_untimed):
    """What the count block and `kbbq count` do before their first table: the prefilter pass (read('prefilter', filter=...)
    over all rows, through a new KmerFilter of filter_words(windows, filter_bits) words, whose `seen` is released after it), the
    number of rounds and the table's size.  Returns (filt, admitted, filter_bytes, P, slots, budget): the filter (None
    without; the caller closes it), its `admitted` (None without) and its bytes during the pass, the rounds that `partitions`
    resolves to, the slots of the table (`slots` when given, else partition_slots for P > 1 and default_slots for P = 1, of
    `admitted` with the prefilter and of `windows` without) and the budget these were taken within -- room's rule, see
    count_block.  A pass that raises closes the filter."""
    from . import _device as dev
    filt, admitted, filter_bytes = None, None, 0
    try:
        if prefilter:
            with stage('k-mer prefilter', sync=True):
                filt = KmerFilter(filter_words(windows, filter_bits))
                read('prefilter', filter=filt)
                filter_bytes, admitted = filt.nbytes, filt.admitted
                filt.release_seen()
        total = admitted if prefilter else int(windows)
        budget = dev.device_budget() if room is None else int(room) - (filt.nbytes if filt is not None else 0)
        P = resolve_partitions(partitions, total, budget) if partitions != 1 else 1
        if slots is None:
            slots = partition_slots(total, P, budget) if P > 1 else default_slots(total, budget)
    except BaseException:
        if filt is not None:
            filt.close()
        raise
    return filt, admitted, filter_bytes, P, slots, budget


def count_block(read, windows, k, min_count=None, slots=None, prefilter=False, filter_bits=4, partitions=1, kmers_from=None,
                room=None, stage=_untimed):
    """The counting block of every k-mer command: prefilter, partitions, table size, the count in one round or in P, the
    histogram and the threshold -- or a k-mer set loaded in the count's place.
    read(what, **kw) runs one pass over ALL rows the caller counts and returns nothing: what = 'prefilter' (kw: filter) is
    kmer's prefilter, what = 'count' (kw: table, filter, parts, part) its count.  What the rows are is the caller's: a host
    plane, a device plane, a gated plane, every band with its gated plane; it frees its gated planes when the block returns.
    windows: what sizes the filter and, without the prefilter, the default table: the caller's k-mer windows (kmer_total,
    batch_windows), or the counted windows of its gate.  slots overrides the table's size.  partitions: checked, an int or 'auto'.
    room: the two budget rules.  None (correct_reads, whose rows are the caller's host or device planes and not the block's
    to account for): the whole device_budget(), read once the filter exists and not reduced by it, and load_set's own default.
    An integer (the commands that keep planes resident beside the table): the device budget less those planes, as the caller
    read and summed them; the filter's `twice` array is taken off it here, and the rest goes to resolve_partitions,
    partition_slots, default_slots, count_partitioned and load_set.
    kmers_from (checked: no counting option goes with it): load_set(kmers_from, min_count, slots, k=k) within that budget.
    stage: recalibrate's stage(name, sync=True) timer for 'k-mer prefilter', 'k-mer count' and 'k-mer load'; nothing is timed without.
    Returns (table, hist, t, info): the table the correct / flag kernels read at min_count = t -- the caller closes it --, its
    histogram (with the prefilter: h[2:]; over all rounds; the file's) and info = {'slots', 'table_bytes', 'filter_bytes',
    'admitted'} plus count_partitioned's keys with more than one round ('slots' and 'table_bytes' are then the per-partition
    table's) or load_set's after a load.  The filter is closed here on every path: before the histogram in one round, after the
    last in several."""
    if kmers_from is not None:
        with stage('k-mer load', sync=True):
            table, hist, t, more = load_set(kmers_from, min_count, slots, k=k, budget=room)
        return table, hist, t, dict(dict(filter_bytes=0, admitted=None), **more)
    filt, admitted, filter_bytes, P, slots, budget = count_plan(read, windows, slots, prefilter, filter_bits, partitions, room, stage)
    table = None
    try:
        if P > 1:
            with stage('k-mer count', sync=True):
                table, hist, t, more = count_partitioned(lambda tab, p: read('count', table=tab, filter=filt, parts=P, part=p),
                                                         k, P, slots, min_count, budget)
        else:
            with stage('k-mer count', sync=True):
                table = KmerTable(k, slots)
                read('count', table=table, filter=filt, parts=1, part=0)
            if filt is not None:                 # before the histogram
                filt.close()
                filt = None
            hist = kmer_histogram(table)
            t = int(min_count) if min_count is not None else solid_threshold(hist)
            more = {}
        if t < 1:
            raise ValueError('min_count must be >= 1, got %d' % t)
        info = dict(dict(slots=table.slots, table_bytes=table.nbytes, filter_bytes=filter_bytes, admitted=admitted), **more)
        done, table = table, None
        return done, hist, t, info
    finally:
        if filt is not None:
            filt.close()
        if table is not None:
            table.close()


def correct_reads(seq_plane, meta, k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, fix_n=False, passes=1,
                  partitions=1, qual_plane=None, kmer_min_qual=None, kmers_from=None):
    """Count, pick the threshold (min_count, else the histogram's first valley) and correct.  Returns (corrected plane in
    the input's layout and kind, info) with info = {'k', 'min_count', 'hist', 'changed' (per read), 'slots', 'table_bytes',
    'prefilter', 'filter_bytes', 'admitted', 'fix_n', 'passes'}.  passes: the rule applied that many times to each row against
    the one table counted from the reads as read (the prefilter composes: the lookups only ask count >= min_count >= 2).  fix_n: Ns are decided by the N rule against the same table (the
    prefilter only keeps keys of count 1 out, and the rule asks for count >= min_count >= 2 then).  With `prefilter` a KmerFilter of `filter_bits` bits per k-mer window and array
    keeps most k-mers seen once out of the table: the same plane, threshold and hist[2:]; hist[1] is the number of once-seen
    k-mers that got in; the table, unless `slots` is given, is sized from the filter's `admitted` after `seen` is freed;
    min_count must be >= 2.  filter_bytes is the filter's size during its pass (both arrays); admitted is None without.
    partitions = P > 1, or 'auto' where partitions_for gives more than 1 (count_partitioned): the k-mers are counted in P rounds
    through a table of `slots` slots (default: partition_slots of the windows -- of `admitted` with the prefilter, whose `twice`
    array lives through all rounds -- in the device budget) and the reads corrected against the solid table of the kept pairs:
    the same plane, changed, min_count and hist (hist[2:] with the prefilter).  info then has 'partitions', 'kept_pairs' and
    'solid_slots' too, and 'slots' / 'table_bytes' describe the per-partition table.  P = 1 is the path without the option.
    kmer_min_qual = Q (with qual_plane, character qualities at offset 33; gate_plane): only the windows whose k bases all have
    quality >= Q are counted.  The prefilter, the count and every partition round read the gated plane, which is freed when the
    count is over; the filter and the default table are sized from the counted windows; the histogram and the threshold are
    the gated table's; the rows as read are corrected against it.  info then has 'kmer_min_qual', 'counted_windows' and
    'windows' (the ungated total) too.
    kmers_from = PATH (load_set): nothing is counted -- the table, the histogram and the threshold are those of the k-mer set file
    (k too: pass k=None, or the file's), and the reads are corrected against it as against a table counted here.  No counting
    option goes with it (check_kmers_from).  info then has 'kmers_from' and 'loaded_kmers' too."""
    passes = check_passes(passes)
    kmers_from = check_kmers_from(kmers_from, prefilter, filter_bits, partitions, kmer_min_qual)
    partitions = _check_partitions(partitions)
    kmer_min_qual = check_kmer_min_qual(kmer_min_qual, qual_plane is not None)
    if prefilter:
        _check_prefilter(min_count, filter_bits)
    windows = kmer_total(_host_meta(meta), k) if kmers_from is None else 0
    rows, gate = [seq_plane, meta], {}                   # the plane and the sidecar the prefilter and the count read
    if kmer_min_qual is not None:
        from . import _device as dev
        d_meta = _to_device(dev._torch(), meta, np.uint32)
        gated, counted = gate_plane(seq_plane, qual_plane, d_meta, k, kmer_min_qual)
        rows, gate = [gated, d_meta], dict(kmer_min_qual=kmer_min_qual, counted_windows=counted, windows=windows)
        del gated

    def read(what, **kw):
        (prefilter_kmers if what == 'prefilter' else count_kmers)(*rows, k=k, **kw)
    table = None
    try:
        table, hist, t, more = count_block(read, gate.get('counted_windows', windows), k, min_count=min_count, slots=slots,
                                           prefilter=prefilter, filter_bits=filter_bits, partitions=partitions, kmers_from=kmers_from)
        del rows[:]                                      # a gated plane is freed here: the correction reads the rows as read
        out, changed = correct_with(table, seq_plane, meta, t, fix_n=fix_n, **_passes_kw(passes))
        return out, dict(dict(k=table.k, min_count=t, hist=hist, changed=changed, prefilter=bool(prefilter), fix_n=bool(fix_n),
                              passes=passes, **gate), **more)
    finally:
        del rows[:]
        if table is not None:
            table.close()


@_bgzf.option
def correct_fastq(path, out, k=31, min_count=None, slots=None, local_slots=None, prefilter=False, filter_bits=4, fix_n=False,
                  passes=1, partitions=1, kmer_min_qual=None, kmers_from=None):
    """Correct every read of a FASTQ file (plain or .gz) and write '@' + name, the corrected sequence, '+' and the qualities
    as read to `out` (a path, or a text stream).  Returns correct_reads' info.  In a process group of several ranks (or of
    one with KBBQ_DIST_ALWAYS=1) this is correct_fastq_ranks, which has no prefilter and no partitions.  kmer_min_qual: the
    quality gate of correct_reads, by the file's own quality lines.  kmers_from: correct_reads' -- the k-mers of a set file in
    the place of the count; under ranks every rank loads the set (correct_fastq_ranks)."""
    passes = check_passes(passes)
    if check_kmers_from(kmers_from, prefilter, filter_bits, partitions, kmer_min_qual, local_slots) is not None:
        if _ranks() is not None:
            return correct_fastq_ranks(path, out, k=k, min_count=min_count, slots=slots, fix_n=fix_n, **_passes_kw(passes),
                                       kmers_from=kmers_from)
    partitions = _check_partitions(partitions)
    kmer_min_qual = check_kmer_min_qual(kmer_min_qual)
    if prefilter:
        _check_prefilter(min_count, filter_bits)
    if _ranks() is not None:
        return correct_fastq_ranks(path, out, k=k, min_count=min_count, slots=slots, local_slots=local_slots, fix_n=fix_n,
                                   **_passes_kw(passes), **_min_qual_kw(kmer_min_qual))
    from . import fastx
    fq = fastx.NativeFastq(path)
    try:
        n, S = fq.scan(None, False)[:2]
        pitch = fastx.pitch_for(S)
        seq, _, qual, meta = fq.fill(None, False, n, pitch)
        names = fq.names()
    finally:
        fq.close()
    fixed, info = correct_reads(seq, meta, k=k, min_count=min_count, slots=slots, prefilter=prefilter, filter_bits=filter_bits,
                                fix_n=fix_n, **_passes_kw(passes), **_partitions_kw(partitions),
                                **_min_qual_kw(kmer_min_qual, qual_plane=qual), **_kmers_from_kw(kmers_from))
    text = fastx.format_fastq(names, fixed, qual, meta & 0xFFFF)
    _write_fastq(out, text)
    info['reads'] = n
    return info


@_bgzf.option
def main_correct(path, output=None, k=31, min_count=None, slots=None, local_slots=None, prefilter=False, filter_bits=4, fix_n=False,
                 passes=1, partitions=1, kmer_min_qual=None, kmers_from=None):
    """`kbbq correct`: the corrected FASTQ to `output` or stdout; the threshold and the changed bases to stderr (once, by rank
    0, with the figures of all ranks); with fix_n ` fix_n=1`; with passes = P > 1 ` passes=P`; with more than one partition
    (given, or resolved from 'auto') ` partitions=P`; with the quality gate ` kmer_min_qual=Q counted_windows=N`; with the
    prefilter also the admitted k-mers and the table's slots; with kmers_from, at the very end, ` kmers_from=1 loaded_kmers=N`."""
    passes = check_passes(passes)                        # every rank refuses, before its first collective
    check_kmers_from(kmers_from, prefilter, filter_bits, partitions, kmer_min_qual, local_slots)   # ... this too
    kmer_min_qual = check_kmer_min_qual(kmer_min_qual)   # ... this too
    partitions = _check_partitions(partitions)           # ... this too: a process group takes no partitions
    if prefilter:
        _check_prefilter(min_count, filter_bits)         # every rank refuses, before its first collective
    ranks = _ranks()
    if ranks is None:
        info = correct_fastq(path, output if output else sys.stdout, k=k, min_count=min_count, slots=slots,
                             prefilter=prefilter, filter_bits=filter_bits, fix_n=fix_n, **_passes_kw(passes),
                             **_partitions_kw(partitions), **_min_qual_kw(kmer_min_qual), **_kmers_from_kw(kmers_from))
        changed = int(np.asarray(info['changed'], dtype=np.int64).sum())
    else:
        try:
            info = correct_fastq_ranks(path, output if output else sys.stdout, k=k, min_count=min_count, slots=slots,
                                       local_slots=local_slots, fix_n=fix_n, **_passes_kw(passes),
                                       **_min_qual_kw(kmer_min_qual), **_kmers_from_kw(kmers_from))
        except Exception as exc:
            if not getattr(exc, 'every_rank', False):
                raise
            # every rank has this error: each says so before any leaves (a launcher ends the job at the first rank that exits)
            from . import parallel
            sys.stderr.write('kbbq correct: rank %d: %s: %s\n' % (ranks[1], type(exc).__name__, exc))
            sys.stderr.flush()
            parallel.barrier()
            sys.exit(1)
        changed = info['changed_bases']
        if ranks[1] != 0:
            return info
    sys.stderr.write(summary_line('correct', dict(info, changed_bases=changed), dict(fix_n=fix_n, passes=passes, prefilter=prefilter)))
    return info


# ---- several ranks ----------------------------------------------------------------------------------------------------------

def _ranks():
    """(world, rank) when this process is a rank of a process group of several (or of one, with KBBQ_DIST_ALWAYS=1), else
    None.  A process that has not imported torch has no process group."""
    from . import parallel
    if parallel._dist() is None:
        return None
    world, rank = parallel.world_rank()
    return (world, rank) if world > 1 or os.environ.get('KBBQ_DIST_ALWAYS') else None


def _agree(exc, index=0):
    """parallel.raise_first_error after a data-dependent step; what it raises is marked as every rank's (main_correct)."""
    from . import parallel
    try:
        parallel.raise_first_error(exc, index)
    except Exception as e:
        e.every_rank = True
        raise


def _rounds(meta, k, cap):
    """Contiguous row ranges [lo, hi) of at most `cap` k-mer windows each (a row with more windows is a range of its own)."""
    w = np.maximum((np.asarray(meta, dtype=np.uint32).astype(np.int64) & 0xFFFF) - k + 1, 0)
    cum = np.cumsum(w)
    out, lo = [], 0
    while lo < len(w):
        before = int(cum[lo - 1]) if lo else 0
        hi = max(int(np.searchsorted(cum, before + cap, side='right')), lo + 1)
        out.append((lo, hi))
        lo = hi
    return out


def count_kmers_ranks(seq_plane, meta, k=31, slots=None, local_slots=None, windows=None, mine=None):
    """This rank's OWNER table: the global count of every k-mer whose owner() is this rank.  Every rank calls it with its own
    rows (host arrays).  The rows are counted into a local table of `local_slots` slots (default: the shard's windows at a
    load factor of 0.5, capped by half the device budget) in rounds of contiguous rows that fit it; after every round the
    occupied slots go to their owners in one exchange and are merged there.  The owner table has `slots` slots (default: the
    global windows / world * 9/8 at a load factor of 0.5, capped by the budget); `windows` is the global number of windows
    (summed over the ranks when None).  A table that fills on any rank raises on every rank.  mine: this rank's windows when
    they are fewer than its sidecars say (a gated shard, whose plane seq_plane then is; the rounds are still cut by the
    sidecars, an upper bound)."""
    from . import _device as dev
    from . import parallel
    world, _ = parallel.world_rank()
    meta = np.ascontiguousarray(meta, dtype=np.uint32)
    if mine is None:
        mine = kmer_total(meta, k)
    if windows is None:
        windows = int(parallel.sum_over_ranks(np.array([mine], dtype=np.int64))[0])
    owned = local = exc = None
    try:
        budget = dev.device_budget()
        if local_slots is None:
            local_slots = default_slots(mine, budget // 2)
        rounds = _rounds(meta, k, max(int(int(local_slots) * LOAD_FACTOR), 1))
        if slots is None:
            slots = default_slots(-(-int(windows) // world) * 9 // 8, budget)
        owned = KmerTable(k, slots)
        if rounds:
            local = KmerTable(k, local_slots)
    except Exception as e:                   # noqa: BLE001 -- every rank must reach the agreement
        exc, rounds = e, []
    _agree(exc)
    nrounds = parallel.max_over_ranks(len(rounds))
    T = dev._torch()
    for i in range(nrounds):
        exc = None
        if i < len(rounds):
            lo, hi = rounds[i]
            try:
                if i:
                    local.clear()
                count_kmers(seq_plane[lo:hi], meta[lo:hi], table=local)
            except Exception as e:           # noqa: BLE001
                exc = e
        _agree(exc)
        if i < len(rounds):
            keys, counts, sizes = select(local, world, 1)
        else:                                # this rank's reads are done: it joins with nothing to send
            keys = T.empty(0, dtype=T.int64, device='cuda')
            counts = T.empty(0, dtype=T.int32, device='cuda')
            sizes = np.zeros(world, dtype=np.int64)
        keys, got = parallel.all_to_all_rows(keys, sizes)
        counts, _ = parallel.all_to_all_rows(counts, sizes, got)
        exc = None
        try:
            merge(owned, keys, counts)
        except Exception as e:               # noqa: BLE001
            exc = e
        del keys, counts
        _agree(exc)
    if local is not None:
        local.close()
    return owned


def kmer_histogram_ranks(table):
    """kmer_histogram of the owner tables of all ranks, summed: the histogram of the whole input."""
    from . import parallel
    return parallel.sum_over_ranks(kmer_histogram(table))


def solid_table(owned, min_count):
    """The k-mers with count >= min_count of every rank's owner table, gathered into a table of their own on every rank (sized
    for them at a load factor of 0.5).  Closes `owned`.  Correcting against it at min_count decides every base as the whole
    table would: a solid key carries its global count, every other key is absent (count 0 < min_count)."""
    from . import _device as dev
    from . import parallel
    keys, counts, _ = select(owned, 1, min_count)
    k = owned.k
    owned.close()
    keys = parallel.all_gather_rows(keys)
    counts = parallel.all_gather_rows(counts)
    table = exc = None
    try:
        table = merge(KmerTable(k, default_slots(int(keys.shape[0]), dev.device_budget())), keys, counts)
    except Exception as e:                   # noqa: BLE001
        exc = e
    _agree(exc)
    return table


def _write_fastq(out, text, ranks=None):
    """The output step of correct_fastq and of the rank paths: `text` to `out`, a path (BGZF with --bgzf, else latin-1 text)
    or a text stream.  ranks = (world, rank) of a process group: a path is `out`.rankNNNN (`out` itself with one rank), a
    stream is written in rank order."""
    if isinstance(out, str):
        path = out if ranks is None or ranks[0] == 1 else '%s.rank%04d' % (out, ranks[1])
        if _bgzf.enabled():
            _bgzf.write_text(path, text)
        else:
            with open(path, 'w', encoding='latin-1', newline='') as fh:
                fh.write(text)
        return

    def write():
        if _bgzf.enabled():
            _bgzf.write_text(out, text)
        else:
            out.write(text)
            out.flush()
    if ranks is None:
        write()
    else:
        from . import parallel
        parallel.in_rank_order(write)


def _correct_shard(table, k, t, hist, reads, out, names, seq, qual, meta, fix_n, passes):
    """What every rank does once it has its table (the gathered solid table, or a loaded set; closed here): correct its own
    rows at min_count = t, agree on an error, sum the changed bases over the ranks and write its records.  Returns the info
    both rank paths start from."""
    from . import fastx
    from . import parallel
    fixed = changed = exc = None
    try:
        fixed, changed = correct_with(table, seq, meta, t, fix_n=fix_n, **_passes_kw(passes))
    except Exception as e:                   # noqa: BLE001 -- every rank must reach the agreement
        exc = e
    finally:
        table.close()
    _agree(exc)
    total = int(parallel.sum_over_ranks(np.array([changed.astype(np.int64).sum()], dtype=np.int64))[0])
    _write_fastq(out, fastx.format_fastq(names, fixed, qual, meta & 0xFFFF), parallel.world_rank())
    return dict(k=k, min_count=t, hist=hist, changed=changed, reads=reads, changed_bases=total, fix_n=bool(fix_n), passes=passes)


def _correct_shard_from(kmers_from, out, names, seq, qual, meta, k, min_count, slots, fix_n, passes):
    """correct_fastq_ranks past its shard with a k-mer set in the place of the count, the gather and the solid table."""
    from . import parallel
    loaded = exc = None
    try:
        loaded = load_set(kmers_from, min_count, slots, k=k)
    except Exception as e:                   # noqa: BLE001 -- every rank must reach the agreement
        exc = e
    try:
        _agree(exc)
    except BaseException:
        if loaded is not None:
            loaded[0].close()
        raise
    table, hist, t, more = loaded
    reads = sum(parallel.all_gather_object(len(names)))
    info = _correct_shard(table, more['k'], t, hist, reads, out, names, seq, qual, meta, fix_n, passes)
    return dict(info, **{key: more[key] for key in ('kmers_from', 'loaded_kmers', 'slots')})


def _read_shard(path, rank, world):
    """(names, seq plane, qual plane, meta) of this rank's records.  A plain file: the records that start in this rank's
    byte range, cut at record starts (kbbq_fastq_sync_offset) -- nobody reads the whole file.  A .gz file: every rank
    inflates all of it and takes parallel.shard_range of the records."""
    from . import fastx
    from . import parallel
    lib = N.load()
    if fastx._is_gzip(path):
        fq = fastx.NativeFastq(path)
    else:
        size = os.path.getsize(path)

        def cut(r):
            if r <= 0 or r >= world:
                return 0 if r <= 0 else size
            off = int(lib.kbbq_fastq_sync_offset(str(path).encode(), size * r // world))
            if off < 0:
                N.check(N.KBBQ_E_ARG)
            return off
        lo_b = cut(rank)
        fq = fastx.NativeFastq.open_range(path, lo_b, max(cut(rank + 1), lo_b), 0, 0)
    try:
        n, S = fq.scan(None, False)[:2]
        lo, hi = parallel.shard_range(n, rank, world) if fastx._is_gzip(path) else (0, n)
        seq, _, qual, meta = fq.fill(None, False, hi - lo, fastx.pitch_for(S), first=lo)
        names = [fq.name(i) for i in range(lo, hi)]
    finally:
        fq.close()
    return names, seq, qual, meta


@_bgzf.option
def correct_fastq_ranks(path, out, k=31, min_count=None, slots=None, local_slots=None, fix_n=False, passes=1, kmer_min_qual=None,
                        kmers_from=None):
    """correct_fastq on every rank of the process group: each rank reads, counts and corrects its own records and writes them
    to `out`.rankNNNN (`out` itself with one rank) or, for a stream, to `out` in rank order.  The threshold comes from the
    global histogram; info carries this rank's per-read changes and the global 'reads' and 'changed_bases'.  fix_n: every rank
    decides its Ns against the gathered solid table at min_count = t, as one process would against the whole table.  passes:
    solidity is all the passes ask of the table too, so the rank files concatenated stay the one-process output.
    kmer_min_qual: every rank gates its own shard before its local count (gate_plane) and its counted windows size the tables;
    info['counted_windows'] is their sum over the ranks, info['windows'] the ungated total.
    kmers_from: nothing is counted and nothing exchanged -- every rank loads the k-mer set (load_set; `slots` is that table's) and
    corrects its own shard against it, so a set counted on one GPU with the prefilter or in partitions serves every rank.  A
    load that fails on any rank is agreed like the other errors here, before a rank corrects anything."""
    from . import parallel
    passes = check_passes(passes)
    kmers_from = check_kmers_from(kmers_from, kmer_min_qual=kmer_min_qual, local_slots=local_slots)
    kmer_min_qual = check_kmer_min_qual(kmer_min_qual)
    world, rank = parallel.world_rank()
    shard = exc = None
    try:
        shard = _read_shard(path, rank, world)
    except Exception as e:                   # noqa: BLE001
        exc = e
    _agree(exc)
    names, seq, qual, meta = shard
    gated = mine = exc = None
    if kmers_from is not None:
        return _correct_shard_from(kmers_from, out, names, seq, qual, meta, k, min_count, slots, fix_n, passes)
    if kmer_min_qual is not None:
        try:
            gated, mine = gate_plane(seq, qual, meta, k, kmer_min_qual)
            gated = gated.cpu().numpy()      # the local count reads host rows, round by round
        except Exception as e:               # noqa: BLE001
            exc = e
        _agree(exc)
    everyone = parallel.all_gather_object((len(names), kmer_total(meta, k)) + (() if gated is None else (mine,)))
    reads, windows = sum(x[0] for x in everyone), sum(x[1] for x in everyone)
    if gated is None:
        owned = count_kmers_ranks(seq, meta, k=k, slots=slots, local_slots=local_slots, windows=windows)
    else:
        counted = sum(x[2] for x in everyone)
        owned = count_kmers_ranks(gated, meta, k=k, slots=slots, local_slots=local_slots, windows=counted, mine=mine)
        del gated
    hist = None
    if min_count is None:
        hist = kmer_histogram_ranks(owned)
        t = solid_threshold(hist)
    else:
        t = int(min_count)
    if t < 1:
        raise ValueError('min_count must be >= 1, got %d' % t)
    info = _correct_shard(solid_table(owned, t), k, t, hist, reads, out, names, seq, qual, meta, fix_n, passes)
    if kmer_min_qual is not None:
        info.update(kmer_min_qual=kmer_min_qual, counted_windows=counted, windows=windows)
    return info
