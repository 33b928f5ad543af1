"""
K-mer sets: the result of a k-mer count as a file (`kbbq count -o SET`), and its way back into a table (`--kmers-from SET`).

The five commands that decide errors from k-mers (`correct`, `recalibrate -c`, `bqsr --kmers`, `recalibrate -b --kmers`,
`benchmark --kmers`) each count their one input and drop the table when they end.  A set is what kmer.count_rounds keeps of
a count -- every (canonical key, count) pair with count >= keep -- and the histogram, so that several files can be counted into
one set, a set counted once can be decided against many times, and a set counted with the prefilter or in partitions on one GPU
can be loaded by every rank of `correct`.

THE FILE (version 1): little-endian, no padding, exactly 2120 + 12 n bytes.

    offset       type       field
    0            char[8]    'KBBQKMER'
    8            u32        version = 1
    12           u32        k (8..32)
    16           u32        keep (>= 1)
    20           u32        min_qual (0: no quality gate, else the --kmer-min-qual of the count)
    24           u64        n, the number of pairs
    32           u64        reads (records read over all inputs)
    40           u64        windows (k-mer windows counted over all inputs: those without a break; with the gate, the gated ones)
    48           u64        key_sum (sum of the keys mod 2^64)
    56           u64        count_sum (sum of the counts mod 2^64)
    64           u64[257]   hist, as kmer.kmer_histogram defines it, with hist[c] = 0 for every c < keep
    2120         u64[n]     canonical keys, strictly ascending as UNSIGNED 64-bit integers
    2120 + 8 n   u32[n]     counts, counts[i] belonging to keys[i]

A pair is in the file iff its exact count over all inputs is >= keep, and n == sum(hist[keep:]).  THE INVARIANT: the bytes are a
function of the multiset of counted windows and of (k, keep, min_qual) alone -- not of --slots, --prefilter, --partitions, the
split of the reads over input files, or thread order.  The keys are sorted for that, and hist is zero below keep for that (the
prefilter's hist[1] varies from run to run).

This module is the header (pack_header / unpack_header), open_set with the refusals that need no device, the writer and the
`kbbq count` driver (count / main_count).  The way back into a table is kmer.load_set, which checks every pair on the device
(kbbq_kmer_check_pairs_dev) before a correcting kernel sees the table.
"""
import os
import struct
import sys

import numpy as np

MAGIC = b'KBBQKMER'
VERSION = 1
HIST = 257
_HEAD = struct.Struct('<8sIIIIQQQQQ')
HEADER_BYTES = _HEAD.size + 8 * HIST          # 2120
PAIR_BYTES = 12
_U64 = (1 << 64) - 1

assert _HEAD.size == 64 and HEADER_BYTES == 2120


def pack_header(k, keep, min_qual, n, reads, windows, key_sum, count_sum, hist):
    """The 2120 header bytes.  hist: 257 counts (hist[c] for c < keep must be 0 already)."""
    hist = np.asarray(hist).astype('<u8')
    if hist.shape != (HIST,):
        raise ValueError('hist must have %d entries, got shape %r' % (HIST, hist.shape))
    return _HEAD.pack(MAGIC, VERSION, int(k), int(keep), int(min_qual), int(n), int(reads), int(windows), int(key_sum) & _U64,
                      int(count_sum) & _U64) + hist.tobytes()


class KmerSet:
    """The header of a k-mer set file: path, k, keep, min_qual, n, reads, windows, key_sum, count_sum (ints) and hist (int64
    [257]).  keys_offset / counts_offset: where the two arrays start in the file."""

    def __init__(self, path, k, keep, min_qual, n, reads, windows, key_sum, count_sum, hist):
        self.path = path
        self.k, self.keep, self.min_qual, self.n, self.reads, self.windows = k, keep, min_qual, n, reads, windows
        self.key_sum, self.count_sum, self.hist = key_sum, count_sum, hist

    @property
    def keys_offset(self):
        return HEADER_BYTES

    @property
    def counts_offset(self):
        return HEADER_BYTES + 8 * self.n

    @property
    def nbytes(self):
        return HEADER_BYTES + PAIR_BYTES * self.n


def unpack_header(buf, path='<bytes>', size=None):
    """A KmerSet from the first 2120 bytes of a file.  ValueError('k-mer set PATH: ...') for everything that can be refused on
    the header alone: a short header, the magic, the version, k, keep, a non-zero hist below keep, n != sum(hist[keep:]) and,
    with `size` (the file's), size != 2120 + 12 n."""
    def bad(what):
        return ValueError('k-mer set %s: %s' % (path, what))
    if len(buf) < HEADER_BYTES:
        raise bad('%d bytes are no header (%d bytes)' % (len(buf), HEADER_BYTES))
    magic, version, k, keep, min_qual, n, reads, windows, key_sum, count_sum = _HEAD.unpack_from(buf, 0)
    if magic != MAGIC:
        raise bad('not a k-mer set (magic %r, not %r)' % (magic, MAGIC))
    if version != VERSION:
        raise bad('version %d, this build reads version %d' % (version, VERSION))
    if not 8 <= k <= 32:
        raise bad('k must be in 8..32, got %d' % k)
    if keep < 1:
        raise bad('keep must be >= 1, got %d' % keep)
    if min_qual > 93:
        raise bad('min_qual must be in 0..93, got %d' % min_qual)
    hist = np.frombuffer(buf, dtype='<u8', count=HIST, offset=_HEAD.size)
    if int(hist.max()) > (1 << 62):
        raise bad('a histogram entry of %d' % int(hist.max()))
    hist = hist.astype(np.int64)
    below = np.flatnonzero(hist[:min(keep, HIST)])
    if below.size:
        raise bad('hist[%d] = %d below keep = %d must be 0' % (int(below[0]), int(hist[below[0]]), keep))
    if n != int(hist[min(keep, HIST):].sum()):
        raise bad('n = %d pairs but sum(hist[%d:]) = %d' % (n, keep, int(hist[min(keep, HIST):].sum())))
    if size is not None and size != HEADER_BYTES + PAIR_BYTES * n:
        raise bad('%d bytes, but n = %d pairs make %d' % (size, n, HEADER_BYTES + PAIR_BYTES * n))
    return KmerSet(path, k, keep, min_qual, n, reads, windows, key_sum, count_sum, hist)


def open_set(path):
    """The KmerSet of a file: its header read and checked (unpack_header, the file's size included).  No device, no library."""
    path = os.fspath(path)
    size = os.path.getsize(path)
    with open(path, 'rb') as fh:
        head = fh.read(HEADER_BYTES)
    return unpack_header(head, path, size)


def set_threshold(hist, keep):
    """kmer.solid_threshold for a set's histogram: the smallest c in max(2, keep)..255 with hist[c] <= hist[c + 1].  Up to
    keep = 2 that IS solid_threshold; hist is zero below a larger keep, which would make a valley of its own there."""
    h = np.asarray(hist)
    for c in range(max(2, int(keep)), 256):
        if h[c] <= h[c + 1]:
            return c
    raise ValueError('the k-mer count histogram has no valley in %d..255: give min_count' % max(2, int(keep)))


def slab_pairs():
    """Pairs of one staging slab: KBBQ_STAGE_MB (default 96) megabytes of 12-byte pairs."""
    env = os.environ.get('KBBQ_STAGE_MB', '')
    mb = int(env) if env.isdigit() and int(env) > 0 else 96
    return max((mb << 20) // PAIR_BYTES, 1)


def write_set(path, k, keep, min_qual, reads, windows, hist, key_sum, count_sum, slabs, n):
    """Write a set to `path`, which must not exist (it is created exclusively, and removed when the writing fails).  slabs(what)
    yields, for what = 'keys' and then for what = 'counts', NumPy arrays (uint64 / uint32) that make up the n sorted keys and
    their counts; host memory is whatever one array takes."""
    done = False
    with open(path, 'xb') as fh:
        try:
            fh.write(pack_header(k, keep, min_qual, n, reads, windows, key_sum, count_sum, hist))
            for what, dtype in (('keys', '<u8'), ('counts', '<u4')):
                wrote = 0
                for part in slabs(what):
                    part = np.ascontiguousarray(part)
                    if part.dtype.kind != 'u' or part.dtype.itemsize != np.dtype(dtype).itemsize:
                        raise ValueError('write_set: %s of %s' % (what, part.dtype))
                    fh.write(part.astype(dtype, copy=False).tobytes())
                    wrote += int(part.shape[0])
                if wrote != n:
                    raise ValueError('write_set: %d %s for n = %d' % (wrote, what, n))
            done = True
        finally:
            if not done:
                fh.close()
                os.unlink(path)


# ---- kbbq count -----------------------------------------------------------------------------------------------------------------

def _launched():
    """Under a launcher (torch.distributed.run sets RANK / WORLD_SIZE) or in a process group: count refuses, before it joins."""
    from . import kmer, parallel
    return parallel.launched_from_env() or kmer._ranks() is not None


def check_count(fastq=(), alignments=(), output=None, k=31, keep=2, prefilter=False, filter_bits=4, partitions=1, kmer_min_qual=None,
                use_oq=False, exclude_flags=0):
    """Everything `kbbq count` refuses before any device call and before a process group is joined or a collective runs.
    Returns (inputs, partitions, kmer_min_qual, exclude_flags): inputs a list of ('fastq' | 'aln', path)."""
    from . import kmer
    from .gatk.bqsr import check_exclude_flags
    if _launched():
        raise ValueError('kbbq count runs on one GPU: a set counted here -- with --prefilter or --partitions where the table does not '
                         'fit -- loads on every rank of `kbbq correct --kmers-from`')
    inputs = [('fastq', os.fspath(p)) for p in (fastq or ())] + [('aln', os.fspath(p)) for p in (alignments or ())]
    if not inputs:
        raise ValueError('kbbq count needs at least one input: -f FASTQ [FASTQ ...] and / or -b ALN [ALN ...]')
    if output is None:
        raise ValueError('kbbq count needs -o SET, the file to write')
    if os.path.lexists(os.fspath(output)):
        raise ValueError('the k-mer set %s exists: kbbq count does not overwrite; give another name' % output)
    if not 8 <= int(k) <= 32:
        raise ValueError('k must be in 8..32, got %d' % int(k))
    if isinstance(keep, bool) or int(keep) != keep or int(keep) < 1:
        raise ValueError('keep must be an integer >= 1, got %r' % (keep,))
    if int(keep) > 0xFFFFFFFF:
        raise ValueError('keep must fit 32 bits, got %d' % int(keep))
    if not alignments and (use_oq or exclude_flags):
        raise ValueError('%s: only with -b (alignments)' % ', '.join(
            flag for flag, v in (('-u/--use-oq', use_oq), ('-F/--exclude-flags', exclude_flags)) if v))
    exclude_flags = check_exclude_flags(exclude_flags)
    partitions = kmer.check_partitions(partitions)
    kmer_min_qual = kmer.check_kmer_min_qual(kmer_min_qual)
    if prefilter:
        if int(keep) < 2:
            raise ValueError('keep must be >= 2 with the prefilter, got %d: k-mers seen once are not counted' % int(keep))
        if not 1 <= int(filter_bits) <= 64:
            raise ValueError('filter_bits must be in 1..64, got %d' % int(filter_bits))
    return inputs, partitions, kmer_min_qual, exclude_flags


class _Input:
    """One input's reads on the host: seq / qual planes (qual None when nothing gates by it), meta (the lengths the kernels
    read: 0 for an excluded record), reads and excluded."""

    def __init__(self, seq, qual, meta, reads, excluded=0):
        self.seq, self.qual, self.meta, self.reads, self.excluded = seq, qual, meta, int(reads), int(excluded)


def _read_fastq(path, need_qual):
    from . import fastx
    fq = fastx.NativeFastq(path)
    try:
        n, S = fq.scan(None, False)[:2]
        seq, _, qual, meta = fq.fill(None, False, n, fastx.pitch_for(S))
    finally:
        fq.close()
    return _Input(seq, qual if need_qual else None, np.ascontiguousarray(meta & 0xFFFF, dtype=np.uint32), n)


def _read_alignments(path, need_qual, use_oq, exclude_flags):
    """Alignments as `bqsr --kmers` counts them: every base of SEQ of every record (soft clips too); a record with FLAG &
    exclude_flags is a row of length 0.  Records of any lengths: counting has no cycle axis."""
    from . import aln, fastx
    planes = ('seq',) + ((('oq' if use_oq else 'qual'),) if need_qual else ())
    b = aln.alignments(path, planes=planes).batch()          # (KBBQ_GPU_BAM=1: a DeviceBatch, kbbq/_bamin.py; else the reader's)
    n = b.n
    if n == 0:
        return _Input(np.zeros((0, 16), np.uint8), np.zeros((0, 16), np.uint8) if need_qual else None, np.zeros(0, np.uint32), 0)
    S = int(b.qlen.max())
    if S > 0xFFFF:
        raise ValueError('%s: records of %d bases: a row holds up to 65535' % (path, S))
    excluded = (b.flag & exclude_flags) != 0
    lens = b.qlen.astype(np.uint32)
    lens[excluded] = 0
    pitch = fastx.pitch_for(max(S, 1))
    take = getattr(b, 'device_plane', b.plane)               # a DeviceBatch's planes stay where the decode left them
    qual = None
    if need_qual:
        have = b.oq_len if use_oq else b.qual_len
        wrong = np.flatnonzero(~excluded & (b.qlen > 0) & (have != b.qlen))
        if wrong.size:
            i = int(wrong[0])
            raise ValueError('%s: record %d (%s) has %d qualities for %d bases: --kmer-min-qual needs a quality for every base%s'
                             % (path, i, b._text(0, i), max(int(have[i]), 0), int(b.qlen[i]),
                                '' if use_oq else ' (-u takes them from the OQ tag)'))
        qual = take(2 if use_oq else 1, pitch)[:n]
    return _Input(take(0, pitch)[:n], qual, lens, n, int(excluded.sum()))


class _Inputs:
    """The inputs of one count, read one after the other, as often as the count passes over them.  One input alone is read
    once and kept (it is the one that would be resident anyway)."""

    def __init__(self, inputs, need_qual, use_oq, exclude_flags):
        self.inputs, self.need_qual, self.use_oq, self.exclude_flags = inputs, need_qual, use_oq, exclude_flags
        self._only = None

    def _read(self, kind, path):
        if kind == 'fastq':
            return _read_fastq(path, self.need_qual)
        return _read_alignments(path, self.need_qual, self.use_oq, self.exclude_flags)

    def __iter__(self):
        if len(self.inputs) == 1:
            if self._only is None:
                self._only = self._read(*self.inputs[0])
            yield self._only
            return
        for kind, path in self.inputs:
            yield self._read(kind, path)


def _counted_plane(inp, k, Q, word=None):
    """(plane, meta) the prefilter and the count read of one input: its host arrays (the host-buffer entry points stage them slab
    by slab), or with the gate the gated device plane beside the device's copy of the lengths."""
    from . import _device as dev
    from . import kmer
    if Q is None or inp.reads == 0:
        if kmer._on_device(inp.seq):                         # a resident plane (kbbq/_bamin.py) takes the device's copy of the lengths
            return inp.seq, kmer._to_device(dev._torch(), inp.meta, np.uint32)
        return inp.seq, inp.meta
    d_meta = kmer._to_device(dev._torch(), inp.meta, np.uint32)
    plane, _ = kmer.gate_plane(inp.seq, inp.qual, d_meta, k, Q, windows=word)
    return plane, d_meta


def _download(T, dev, src, n, dtype, pairs):
    """The n elements of the device tensor `src` as NumPy arrays of at most `pairs` elements through one page-locked slab."""
    size = np.dtype(dtype).itemsize
    buf = dev.pinned('kmerset', 0, max(min(n, pairs), 1) * 8)
    for lo in range(0, n, pairs):
        m = min(pairs, n - lo)
        host = buf[:m * size].view(T.int64 if size == 8 else T.int32)
        host.copy_(src[lo:lo + m])
        yield host.numpy().view(dtype)


def count(fastq=(), alignments=(), output=None, k=31, keep=2, slots=None, prefilter=False, filter_bits=4, partitions=1,
          kmer_min_qual=None, use_oq=False, exclude_flags=0, histo=None, slab=None):
    """`kbbq count`: count the k-mers of every input into ONE table, one input resident at a time, and write the pairs with count
    >= keep as a k-mer set to `output`.  FASTQ inputs are counted as `kbbq correct` counts them, alignments as `bqsr --kmers`
    does (every base of SEQ; exclude_flags leaves records out; use_oq: the OQ tag is the quality kmer_min_qual gates by).
    prefilter: the filter pass runs over all inputs, then the count over all inputs; partitions = P | 'auto': every round runs
    over all inputs (the files are read again for every pass when there are several); kmer_min_qual: every input is gated in
    front of each pass (kmer.gate_plane).  After the count -- after every round -- kmer.select(table, 1, keep) keeps the pairs;
    the table is freed, all kept pairs are sorted by unsigned key on the device (kbbq_kmer_sort_pairs_dev), checked and summed
    there (kbbq_kmer_check_pairs_dev: what a loader will ask of them) and written slab by slab through page-locked staging:
    host memory does not grow with n.  histo: a file of `c<TAB>hist[c]` lines, c = keep..256 (the last is the >= 256 bin).
    slab: pairs per staging slab (default: KBBQ_STAGE_MB).  Returns info: k, keep, inputs, reads, excluded_reads, windows (every
    window of every read, kmer.kmer_total: what the line on stderr prints), counted_windows (the windows that were inserted --
    without a break and, with the gate, of bases at or above it: the header's `windows`, kmer.count_windows / gate_plane),
    kmers, valley (None when the histogram has none at or above keep), hist, slots, partitions, prefilter, admitted, key_sum,
    count_sum, and with the gate kmer_min_qual."""
    inputs, partitions, Q, exclude_flags = check_count(fastq, alignments, output, k, keep, prefilter, filter_bits, partitions,
                                                       kmer_min_qual, use_oq, exclude_flags)
    from . import _device as dev
    from . import kmer
    k, keep = int(k), int(keep)
    T = dev._torch()
    source = _Inputs(inputs, Q is not None, use_oq, exclude_flags)
    # pass 0: the reads and the windows of all inputs, and the windows a count will insert -- those without a break, with the
    # gate those it leaves -- which go into the header and size the filter and the table
    reads = excluded = windows = 0
    word = T.zeros(1, dtype=T.int64, device='cuda')
    for inp in source:
        reads += inp.reads
        excluded += inp.excluded
        windows += kmer.kmer_total(inp.meta, k)
        if inp.reads and Q is not None:
            kmer.gate_plane(inp.seq, inp.qual, inp.meta, k, Q, windows=word)
        elif inp.reads:
            kmer.count_windows(inp.seq, inp.meta, k, windows=word)
    counted = int(word.cpu().numpy()[0])
    del word

    def read(what, **kw):
        for inp in source:
            if inp.reads:
                plane, meta = _counted_plane(inp, k, Q)
                (kmer.prefilter_kmers if what == 'prefilter' else kmer.count_kmers)(plane, meta, k=k, **kw)
                del plane, meta
    filt, admitted, _, P, slots, _ = kmer.count_plan(read, counted, slots, prefilter, filter_bits, partitions)
    try:
        hist, kept, rounds = kmer.count_rounds(lambda table, p: read('count', table=table, filter=filt, parts=P, part=p), k, P,
                                               slots, keep)
    finally:
        if filt is not None:
            filt.close()
    nslots = rounds['slots']
    hist[:min(keep, HIST)] = 0
    n = sum(int(keys.shape[0]) for keys, _ in kept)
    if n != int(hist[min(keep, HIST):].sum()):
        raise RuntimeError('kbbq count: %d pairs kept but the histogram has %d at or above keep = %d'
                           % (n, int(hist[min(keep, HIST):].sum()), keep))
    keys, counts = kmer.sort_pairs(kept, k)
    del kept
    sums, bad = kmer.check_pairs(keys, counts, k, keep)
    if bad is not None:
        raise RuntimeError('kbbq count: the sorted pairs do not pass their own check: pair %d: %s' % bad)
    pairs = int(slab) if slab else slab_pairs()
    write_set(output, k, keep, Q or 0, reads, counted, hist, int(sums[0]), int(sums[1]),
              lambda what: _download(T, dev, keys if what == 'keys' else counts, n, np.uint64 if what == 'keys' else np.uint32, pairs),
              n)
    del keys, counts
    dev.release_pinned('kmerset')
    if histo is not None:
        with open(histo, 'w') as fh:
            fh.write(''.join('%d\t%d\n' % (c, int(hist[c])) for c in range(min(keep, HIST - 1), HIST)))
    try:
        valley = set_threshold(hist, keep)
    except ValueError:
        valley = None
    info = dict(k=k, keep=keep, inputs=len(inputs), reads=reads, excluded_reads=excluded, windows=windows, kmers=n, valley=valley,
                hist=hist, slots=nslots, partitions=P, prefilter=bool(prefilter), admitted=admitted, key_sum=int(sums[0]),
                count_sum=int(sums[1]), counted_windows=counted)
    if Q is not None:
        info.update(kmer_min_qual=Q)
    return info


def count_line(info, exclude_flags=0):
    """The one stderr line of `kbbq count`."""
    from . import kmer
    return ('kbbq count: k=%d keep=%d inputs=%d reads=%d%s windows=%d kmers=%d valley=%s%s%s%s'
            % (info['k'], info['keep'], info['inputs'], info['reads'],
               ' excluded_reads=%d' % info['excluded_reads'] if exclude_flags else '', info['windows'], info['kmers'],
               'none' if info['valley'] is None else '%d' % info['valley'], kmer.partitions_field(info), kmer.min_qual_field(info),
               ' prefilter=1 admitted=%d slots=%d' % (info['admitted'], info['slots']) if info['prefilter'] else ''))


def main_count(fastq=(), alignments=(), output=None, exclude_flags=0, **kw):
    """`kbbq count`: count() and its line on stderr."""
    info = count(fastq, alignments, output, exclude_flags=exclude_flags, **kw)
    sys.stderr.write(count_line(info, exclude_flags) + '\n')
    return info
