"""
`--bam-index`: the BAI or CSI index of a `--bam-out` file, from what is on the device while the file is written
(include/kbbq_hip.h "BAM index" states the index; csrc/kbbq_bam_index.h reduces a slab; tests/bam_index_model.py is the
executable model).

kbbq/_bamout.py's BamWriter drives an Index: per slab the runs of one (refID, bin) that kbbq_bam_index_dev sends back -- 32 bytes
a run, in offsets of the uncompressed stream -- and the compressed sizes of the blocks as they are written (coff, one entry per
65280 bytes of stream, from BSIZE of the packed bytes); at close() the file-long linear array comes down once, offsets become
virtual offsets, neighbouring chunks of a bin that meet in one compressed block are merged, and the file is serialised.  What is
refused -- a reference too long for BAI, records out of coordinate order, a record beyond the index's reach -- is refused on the
host from the reader's arrays, before the output file exists (resolve, check).
"""
import struct

import numpy as np

from ._bgzf import BLOCK

MIN_SHIFT = 14
BAI_MAX = 1 << 29
KINDS = ('auto', 'bai', 'csi')
RUN = np.dtype([('ref', '<i4'), ('bin', '<u4'), ('beg', '<u8'), ('end', '<u8'), ('n_mapped', '<u4'), ('n_unmapped', '<u4')])
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def references(header):
    """[(SN, LN, the @SQ line)] of a header's lines, in order."""
    refs = []
    for line in header:
        if line.startswith('@SQ'):
            f = dict(x.split(':', 1) for x in line.split('\t')[1:] if ':' in x)
            refs.append((f.get('SN', ''), int(f.get('LN', 0)), line))
    return refs


def depth_for(longest):
    """The smallest depth >= 5 with 2^(14 + 3 * depth) >= longest."""
    depth = 5
    while (1 << (MIN_SHIFT + 3 * depth)) < longest:
        depth += 1
    return depth


def resolve(kind, header):
    """(format, depth) of `kind` (auto, bai, csi) for a header's @SQ lines.  ValueError naming the line for bai with an LN over 2^29."""
    if kind not in KINDS:
        raise ValueError('--bam-index: one of %s, got %r' % (', '.join(KINDS), kind))
    refs = references(header)
    long_ = [line for _, ln, line in refs if ln > BAI_MAX]
    if kind == 'bai' and long_:
        raise ValueError('--bam-index bai: a BAI index reaches 2^29 = 536870912 bases, this reference is longer: %s (--bam-index csi, '
                         'or auto)' % long_[0].replace('\t', ' '))
    if kind == 'bai' or (kind == 'auto' and not long_):
        return 'bai', 5
    return 'csi', depth_for(max([ln for _, ln, _ in refs], default=0))


def index_path(output, fmt):
    return '%s.%s' % (output, fmt)


def window_counts(lengths):
    """ceil(max(LN, 1) / 16384) + 1 windows per reference."""
    return [(max(int(ln), 1) + (1 << MIN_SHIFT) - 1 >> MIN_SHIFT) + 1 for ln in lengths]


def check(bam, depth, lo=0, hi=None):
    """What an index cannot be made of, of alignments [lo, hi) of an aln.AlignmentFile, from the reader's arrays: records out of
    coordinate order -- the key (refID as unsigned, so '*' sorts last; pos) must not decrease in file order, whatever @HD SO: says
    -- or a record that ends beyond 2^(14 + 3 * depth).  ValueError naming the first such alignment, with .read_index."""
    b = bam.batch()
    hi = len(bam) if hi is None else hi
    if hi - lo <= 0:
        return
    index = {name: i for i, (name, _, _) in enumerate(references(bam.header))}
    of_contig = np.array([index.get(name, -1) for name in b.contig_names] + [-1], dtype=np.int64)
    ref = of_contig[b.contig[lo:hi]]
    pos = b.pos[lo:hi].astype(np.int64)
    key = (ref.astype(np.uint32).astype(np.uint64) << np.uint64(32)) + (pos + 1).clip(0).astype(np.uint64)
    down = np.flatnonzero(key[1:] < key[:-1])
    span = np.where((b.flag[lo:hi] & 4) != 0, 0, b.ref_span[lo:hi].astype(np.int64))
    far = np.flatnonzero((ref >= 0) & (pos.clip(0) + span.clip(1) > (1 << (MIN_SHIFT + 3 * depth))))
    first_down = lo + int(down[0]) + 1 if down.size else None
    first_far = lo + int(far[0]) if far.size else None
    if first_down is None and first_far is None:
        return
    if first_far is None or (first_down is not None and first_down < first_far):
        exc = ValueError('alignment %d is out of coordinate order (it sorts before alignment %d): --bam-index needs its input sorted '
                         'by coordinate (samtools sort), or write without the option' % (first_down, first_down - 1))
        exc.read_index = first_down
    else:
        exc = ValueError('alignment %d ends beyond 2^%d, the reach of the index: its reference is longer than the @SQ lines say'
                         % (first_far, MIN_SHIFT + 3 * depth))
        exc.read_index = first_far
    raise exc


def block_sizes(packed):
    """The compressed sizes of the BGZF members of `packed` (BSIZE + 1 of each)."""
    view = memoryview(packed)
    sizes, at, n = [], 0, len(view)
    while at < n:
        size = (view[at + 16] | view[at + 17] << 8) + 1
        sizes.append(size)
        at += size
    return sizes


class Index:
    """The index of one file: runs(...) per slab, blocks(...) per piece of compressed bytes, data(...) at the end."""

    def __init__(self, fmt, depth, lengths):
        self.fmt, self.depth, self.n_ref = fmt, int(depth), len(lengths)
        self.lin_off = np.zeros(self.n_ref + 1, dtype=np.uint64)
        self.lin_off[1:] = np.cumsum(np.array(window_counts(lengths), dtype=np.uint64))
        self._runs = []                                  # arrays of RUN, in file order; the last run of the last array is open
        self._sizes = []
        self.n_runs = 0

    def runs(self, runs):
        """A slab's runs: the first joins the last of the slab before when (refID, bin) agree."""
        if not len(runs):
            return
        runs = np.array(runs, dtype=RUN)
        if self._runs:
            last = self._runs[-1][-1:]
            if last['ref'][0] == runs['ref'][0] and last['bin'][0] == runs['bin'][0]:
                last['end'] = runs['end'][0]
                last['n_mapped'] += runs['n_mapped'][0]
                last['n_unmapped'] += runs['n_unmapped'][0]
                runs = runs[1:]
        if len(runs):
            self._runs.append(runs)
            self.n_runs += len(runs)

    def blocks(self, packed):
        self._sizes.extend(block_sizes(packed))

    def pseudo_bin(self):
        return 37450 if self.fmt == 'bai' else ((1 << (3 * self.depth + 3)) - 1) // 7 + 1

    def data(self, linear, eof_at):
        """The index's bytes (CSI: before compression).  linear: the file-long linear array in stream offsets, all ones where
        empty; eof_at: the file offset of the EOF block."""
        coff = np.zeros(len(self._sizes) + 1, dtype=np.uint64)
        coff[1:] = np.cumsum(np.array(self._sizes, dtype=np.uint64))
        if int(coff[-1]) != int(eof_at):
            raise RuntimeError('--bam-index: %d bytes of blocks were seen, the EOF block lies at %d' % (int(coff[-1]), eof_at))

        def voffset(u):
            u = np.asarray(u, dtype=np.uint64)
            return coff[(u // np.uint64(BLOCK)).astype(np.int64)] << np.uint64(16) | u % np.uint64(BLOCK)

        runs = np.concatenate(self._runs) if self._runs else np.zeros(0, dtype=RUN)
        placed = runs[runs['ref'] >= 0]
        no_coor = runs[runs['ref'] < 0]
        n_no_coor = int(no_coor['n_mapped'].astype(np.int64).sum() + no_coor['n_unmapped'].astype(np.int64).sum())
        # chunks: the runs by (refID, bin), file order kept within a bin; a chunk begins where the bin changes or the blocks part
        order = np.lexsort((np.arange(len(placed)), placed['bin'], placed['ref']))
        placed_sorted = placed[order]
        beg, end = voffset(placed_sorted['beg']), voffset(placed_sorted['end'])
        key = placed_sorted['ref'].astype(np.int64) << 32 | placed_sorted['bin'].astype(np.int64)
        first_of_bin = np.ones(len(key), dtype=bool)
        first_of_bin[1:] = key[1:] != key[:-1]
        first_of_chunk = first_of_bin.copy()
        first_of_chunk[1:] |= (end[:-1] >> np.uint64(16)) < (beg[1:] >> np.uint64(16))
        chunk_at = np.flatnonzero(first_of_chunk)
        chunk_beg = beg[chunk_at]
        chunk_end = end[np.append(chunk_at[1:], len(key)) - 1] if len(key) else end
        chunk_key = key[chunk_at]
        bin_at = np.flatnonzero(first_of_bin[chunk_at])                  # per bin: its first chunk
        bin_key = chunk_key[bin_at]
        bin_hi = np.append(bin_at[1:], len(chunk_at))
        pairs = np.empty((len(chunk_at), 2), dtype='<u8')
        pairs[:, 0], pairs[:, 1] = chunk_beg, chunk_end
        # the linear array: voffsets, per reference the backfilled windows up to the last non-empty one
        linear = np.asarray(linear, dtype=np.uint64)
        filled = linear != EMPTY
        lin_v = np.zeros(len(linear), dtype=np.uint64)
        lin_v[filled] = voffset(linear[filled])
        out = [b'BAI\1' if self.fmt == 'bai' else b'CSI\1' + struct.pack('<iii', MIN_SHIFT, self.depth, 0), struct.pack('<i', self.n_ref)]
        bin_ref = bin_key >> 32
        ref_lo = np.searchsorted(bin_ref, np.arange(self.n_ref), 'left')
        ref_hi = np.searchsorted(bin_ref, np.arange(self.n_ref), 'right')
        run_lo = np.searchsorted(placed['ref'], np.arange(self.n_ref), 'left')          # (file order is reference order: check)
        run_hi = np.searchsorted(placed['ref'], np.arange(self.n_ref), 'right')
        have = np.flatnonzero(filled)
        have_lo, have_hi = np.searchsorted(have, self.lin_off[:-1], 'left'), np.searchsorted(have, self.lin_off[1:], 'left')
        nothing = struct.pack('<i', 0) + (struct.pack('<i', 0) if self.fmt == 'bai' else b'')
        for ref in range(self.n_ref):
            if run_lo[ref] == run_hi[ref] and have_lo[ref] == have_hi[ref]:
                out.append(nothing)
                continue
            lo, hi = int(self.lin_off[ref]), int(self.lin_off[ref + 1])
            n_intv = int(have[have_hi[ref] - 1]) - lo + 1 if have_hi[ref] > have_lo[ref] else 0
            back = lin_v[lo:lo + n_intv].copy()
            if n_intv:
                at = np.where(filled[lo:lo + n_intv], np.arange(n_intv), n_intv)
                back = back[np.minimum.accumulate(at[::-1])[::-1]]
            of_ref = placed[int(run_lo[ref]):int(run_hi[ref])]
            nbins = int(ref_hi[ref] - ref_lo[ref])
            out.append(struct.pack('<i', nbins + (1 if len(of_ref) else 0)))
            for k in range(int(ref_lo[ref]), int(ref_hi[ref])):
                number = int(bin_key[k] & 0xFFFFFFFF)
                chunks = pairs[int(bin_at[k]):int(bin_hi[k])]
                if self.fmt == 'bai':
                    out.append(struct.pack('<Ii', number, len(chunks)))
                else:
                    out.append(struct.pack('<IQi', number, self._loffset(number, back, hi - lo), len(chunks)))
                out.append(chunks.tobytes())
            if len(of_ref):
                meta = struct.pack('<QQQQ', int(voffset(of_ref['beg'][0])), int(voffset(of_ref['end'][-1])),
                                   int(of_ref['n_mapped'].astype(np.int64).sum()), int(of_ref['n_unmapped'].astype(np.int64).sum()))
                out.append(struct.pack('<Ii', self.pseudo_bin(), 2) if self.fmt == 'bai' else struct.pack('<IQi', self.pseudo_bin(), 0, 2))
                out.append(meta)
            if self.fmt == 'bai':
                out.append(struct.pack('<i', n_intv))
                out.append(back.astype('<u8').tobytes())
        out.append(struct.pack('<Q', n_no_coor))
        return b''.join(out)

    def _loffset(self, number, back, windows):
        """The backfilled linear value at the first 16 kb window of bin `number` (clamped to the reference's last window)."""
        level, first = 0, 0
        while number >= first + (1 << (3 * level)):
            first += 1 << (3 * level)
            level += 1
        window = (number - first) << (3 * (self.depth - level))
        window = min(window, windows - 1)
        return int(back[window]) if window < len(back) else 0
