"""
Case generator and expected values for the aligned-read kernels (K4 kbbq_find_errors_dev, K5 kbbq_count_q_dev,
K6 kbbq_canonical_reads_dev).  No GPU, no torch: numpy and the CPU oracle only.

A `World` is a genome of ACGT bytes and a site mask.  A `Read` is built along its CIGAR from the genome (inserted and
clipped bases random, substitutions on a quarter of the bases) and carries the attributes oracle_benchmark.find_read_errors
reads.  The expected flags are that function's, flipped for reverse reads as oracle_benchmark.get_error_dict flips them; for
a read it raises on, the expected value is the exception class.  `csr` lays reads out as the arrays kbbq_find_errors_dev takes.

The case families walk one operation boundary through every position of a 16-byte chunk, on both strands, in the interior of
the genome and at both of its ends; `long_rows` does the same on rows of more than 4096 bases (more than 256 chunks).
"""
import numpy as np

import oracle_benchmark as OB

M, I, D, N, S, H, P, EQ, X = range(9)
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
CONTIG = 'g'
SHORT_N = (37, 48)
LONG_N = (4097, 4112, 4113, 16400, 33000, 65535)
LONG_GENOME = 70000
READ_CONSUMING = (M, I, S, EQ, X)
REF_CONSUMING = (M, D, N, EQ, X)


class World:
    """Genome (uint8 ACGT) and site mask (uint8 0 / 1): about 30 % of the sites set, independent per base, plus a few runs
    of 20 or more masked and of 20 or more unmasked bases."""

    def __init__(self, G, seed, runs=6):
        rng = np.random.default_rng(seed)
        self.G = G
        self.genome = rng.choice(ACGT, size=G)
        mask = rng.random(G) < 0.3
        for k in range(runs):
            at, l = int(rng.integers(0, G - 40)), int(rng.integers(20, 41))
            mask[at:at + l] = bool(k & 1)
            mask[at + l] |= not k & 1                          # an unmasked run ends on a masked site
        self.mask = mask.astype(np.uint8)
        self.fused = self.genome | (self.mask << 7)           # the site flag in bit 7 of the genome byte

    def dicts(self):
        return {CONTIG: self.genome}, {CONTIG: self.mask.astype(bool)}


class Read:
    """What oracle_benchmark.find_read_errors reads of an alignment, and the strand."""
    reference_name = CONTIG

    def __init__(self, seq, ops, ref_start, ref_len, reverse, family=''):
        self.seq = np.asarray(seq, dtype=np.uint8)
        self.query_sequence = self.seq.tobytes().decode('ascii')
        self.cigartuples = [(int(o), int(l)) for o, l in ops]
        self.reference_start, self.reference_end = int(ref_start), int(ref_start) + int(ref_len)
        self.is_reverse = bool(reverse)
        self.family = family
        self._flags = None

    def __len__(self):
        return len(self.seq)

    def __str__(self):
        return '%s %s @%d%s' % (self.family, cigar_text(self.cigartuples), self.reference_start, ' reverse' if self.is_reverse else '')


def cigar_text(ops):
    return ''.join('%d%s' % (l, 'MIDNSHP=X????? ?'[o]) for o, l in ops)


def read_len(ops):
    return sum(l for o, l in ops if o in READ_CONSUMING)


def ref_span(ops):
    return sum(l for o, l in ops if o in REF_CONSUMING)


def build_read(world, ops, ref_start, reverse, rng, family='', ref_len=None, nbases=None):
    """The read along its CIGAR from the genome at ref_start: M / = / X copy the reference, I / S draw random bases, then a
    quarter of all bases are replaced by ANOTHER letter.  ref_len / nbases: what the record claims when that is not what the
    operations add up to (the shapes the reference raises on)."""
    parts, g = [], int(ref_start)
    for o, l in ops:
        if o in (M, EQ, X):
            have = world.genome[g:g + l]
            parts.append(np.concatenate([have, rng.choice(ACGT, size=l - len(have))]))
            g += l
        elif o in (I, S):
            parts.append(rng.choice(ACGT, size=l))
        elif o in (D, N):
            g += l
    seq = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    if nbases is not None:
        seq = seq[:nbases]
    sub = rng.random(len(seq)) < 0.25
    code = np.searchsorted(ACGT, seq)
    seq = np.where(sub, ACGT[(code + rng.integers(1, 4, size=len(seq))) % 4], seq).astype(np.uint8)
    return Read(seq, ops, ref_start, ref_span(ops) if ref_len is None else ref_len, reverse, family)


def expected(read, world, flip=True):
    """(errors, skips) as bool arrays in the orientation K4 writes them (reversed for a reverse read when `flip`), or the
    class of the exception the reference raises."""
    if read._flags is None:
        ref, var = world.dicts()
        try:
            read._flags = OB.find_read_errors(read, ref, var)
        except Exception as e:                                   # noqa: BLE001  (the class IS the expected value)
            read._flags = type(e)
    f = read._flags
    if isinstance(f, type):
        return f
    return (np.flip(f[0]), np.flip(f[1])) if (flip and read.is_reverse) else f


def pitch_for(reads):
    return max(16, (max(len(r) for r in reads) + 15) // 16 * 16)


def csr(reads, pitch=None):
    """The arrays kbbq_find_errors_dev takes: seq[n, pitch], len, ref_start, ref_len, cig_off, cig_n, cigar = len << 4 | op, flip."""
    n = len(reads)
    pitch = pitch_for(reads) if pitch is None else pitch
    seq = np.zeros((n, pitch), dtype=np.uint8)
    cigar, cig_off, cig_n = [], np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, r in enumerate(reads):
        seq[i, :len(r)] = r.seq
        cig_off[i], cig_n[i] = len(cigar), len(r.cigartuples)
        cigar += [(l << 4) | o for o, l in r.cigartuples]
    return dict(n=n, pitch=pitch, seq=seq, len=np.array([len(r) for r in reads], dtype=np.uint32),
                ref_start=np.array([r.reference_start for r in reads], dtype=np.int64),
                ref_len=np.array([r.reference_end - r.reference_start for r in reads], dtype=np.int32),
                cig_off=cig_off, cig_n=cig_n, cigar=np.array(cigar + [0], dtype=np.uint32),
                flip=np.array([r.is_reverse for r in reads], dtype=np.uint8))


def expected_planes(reads, world, pitch, flip=True):
    """(err, skip) uint8 [n, pitch]: the expected flags inside every read, 0 behind it."""
    err = np.zeros((len(reads), pitch), dtype=np.uint8)
    skip = np.zeros_like(err)
    for i, r in enumerate(reads):
        e, s = expected(r, world, flip)
        err[i, :len(r)], skip[i, :len(r)] = e, s
    return err, skip


# ---------------------------------------------------------------- families of CIGAR shapes (lists of operation lists)
def insertion_shapes():
    """bM lI restM for every b and the lengths that leave the second M inside / on the edge of / outside the chunk."""
    return [[(M, b), (I, l), (M, n - b - l)] for n in SHORT_N for b in range(1, n - 1) for l in (1, 2, 3, 15, 16, 17) if n - b - l >= 1]


def deletion_shapes():
    """bM lD restM and bM lN restM: with b this takes dat + 1 + dlen through 15, 16, 17 and 18 at every dat."""
    return [[(M, b), (op, l), (M, n - b)] for n in SHORT_N for op in (D, N) for b in range(1, n) for l in (1, 2, 7, 14, 15, 16, 17, 40)]


def soft_clip_shapes():
    out = []
    for n in SHORT_N:
        out += [[(S, a), (M, n - a)] for a in range(1, 18)]
        out += [[(M, n - a), (S, a)] for a in range(1, 18)]
        out += [[(S, a), (M, n - a - c), (S, c)] for a in range(1, 18) for c in range(1, 18)]
    return out


def four_operation_shapes():
    out = []
    for n in SHORT_N:
        out += [[(S, a), (M, b), (D, l), (M, n - a - b)] for a in (1, 16, 17) for b in range(1, n - a) for l in (1, 15, 16)]
        out += [[(M, b), (I, l), (M, c), (S, n - b - l - c)] for b in range(1, n - 3) for l in (1, 16) for c in (1, 13, 16)
                if n - b - l - c >= 1]
    return out


def order_shapes():
    """D before I (the insertion's left neighbour is the last deleted site), I before D (the deletion targets an inserted
    base), D then N (two deletions on one base)."""
    out = []
    for n in SHORT_N:
        for b in range(1, n - 3):
            for l in (1, 3, 15):
                out.append([(M, b), (D, l), (I, 2), (M, n - b - 2)])
                out.append([(M, b), (I, 2), (D, l), (M, n - b - 2)])
                out.append([(M, b), (D, l), (N, 2), (M, n - b)])
    return out


def wrap_shapes():
    """Python's index -1 (a leading deletion marks the LAST base, a leading insertion looks at the LAST site of the window),
    operations that consume nothing, operations of length 0."""
    out = []
    for n in SHORT_N:
        out += [[(D, l), (M, n)] for l in (1, 2, 15, 16, 17)]
        out += [[(N, l), (M, n)] for l in (1, 16)]
        out += [[(I, l), (M, n - l)] for l in (1, 2, 15, 16, 17)]
        for b in range(1, n):
            out.append([(H, 2), (M, b), (P, 2), (D, 1 + b % 4), (M, n - b), (H, 3)])
            out.append([(M, b), (D, 0), (M, n - b)])
            out.append([(M, b), (I, 0), (M, n - b)])
        out.append([(M, 0), (M, n)])
    return out


def eq_x_shapes():
    """A sample of the shapes above with = / X in place of M."""
    out = []
    for fam in (insertion_shapes(), deletion_shapes(), soft_clip_shapes(), four_operation_shapes(), order_shapes()):
        for k, ops in enumerate(fam[::7]):
            out.append([((EQ if (k + i) & 1 else X) if o == M else o, l) for i, (o, l) in enumerate(ops)])
    return out


def walked_shapes():
    """More than four operations: every chunk takes the sequential walk."""
    out = []
    for n in SHORT_N:
        for a in range(1, n - 8, 2):
            for b in (1, 5):
                out.append([(M, a), (I, 2), (M, b), (D, 3), (M, n - a - b - 2)])
        for k in range(12):
            cuts = np.sort(np.random.default_rng(900 + 100 * n + k).choice(np.arange(1, n), size=5, replace=False))
            out.append([(M, int(x)) for x in np.diff(np.concatenate([[0], cuts, [n]]))])
    return out


FAMILIES = dict(insertion=insertion_shapes, deletion=deletion_shapes, soft_clip=soft_clip_shapes, four_operations=four_operation_shapes,
                order=order_shapes, wraps=wrap_shapes, eq_x=eq_x_shapes, walked=walked_shapes)
SHORT_GENOME = 3000


def place(world, shapes, rng, family):
    """Every shape in the interior of the genome on both strands; every fourth also at ref_start = 0 and with its reference
    window ending at the last genome byte."""
    reads = []
    for k, ops in enumerate(shapes):
        span = ref_span(ops)
        starts = [int(rng.integers(20, world.G - span - 20))]
        if k % 4 == 0:
            starts += [0, world.G - span]
        for st in starts:
            for rev in (False, True):
                reads.append(build_read(world, ops, st, rev, rng, family))
    return reads


def short_world():
    return World(SHORT_GENOME, 20260)


def deletion_window_edge(read):
    """(dat + 1 + dlen, first deleted site) of a forward bM lD restM read: dat = the target base's offset in its 16-byte chunk."""
    (_, b), (_, l), _ = read.cigartuples
    return (b - 1) % 16 + 1 + l, read.reference_start + b


def deletion_edge_reads(world, rng):
    """bM lD restM with dat + 1 + dlen = 15, 16, 17, 18 placed where ONLY THE LAST deleted site is masked (and the target base's
    own site is not): whether the target base is skipped hangs on the one site at the edge of / just outside its 16-byte window."""
    reads, n = [], 37
    zeros = np.flatnonzero(world.mask == 0)
    for b in range(1, n):
        for l in (1, 2, 7, 14, 15, 16, 17):
            if not 15 <= (b - 1) % 16 + 1 + l <= 18:
                continue
            for p in zeros + 1:                                          # p - 1: the target base's site, p: the first deleted site
                if p - b >= 0 and p + l + n < world.G and not world.mask[p:p + l - 1].any() and world.mask[p + l - 1]:
                    for rev in (False, True):
                        reads.append(build_read(world, [(M, b), (D, l), (M, n - b)], int(p) - b, rev, rng, 'deletion'))
                    break
            else:
                raise AssertionError('no site pattern for a %d-base deletion' % l)
    return reads


def short_families(world):
    """{family: [Read]}: the same reads on every call (fixed seeds)."""
    fams = {name: place(world, fn(), np.random.default_rng(7000 + i), name) for i, (name, fn) in enumerate(FAMILIES.items())}
    fams['deletion'] += deletion_edge_reads(world, np.random.default_rng(7100))
    return fams


def raising_reads(world):
    """Shapes the reference raises on: each its own launch (a status word fails a whole batch)."""
    rng = np.random.default_rng(4242)
    G = world.G
    mk = lambda ops, st, **kw: build_read(world, ops, st, False, rng, 'raising', **kw)
    return [
        mk([(M, 20), (I, 3)], 100),                                     # insertion as the last reference-consuming operation
        mk([(M, 16), (I, 1)], 200),
        mk([(M, 5), (I, 2), (S, 4)], 300),
        mk([(S, 3), (M, 30), (I, 16), (H, 2)], 400),
        mk([(I, 4)], 500),                                              # ... and with an empty reference window
        mk([(M, 37)], G - 30, ref_len=30),                              # an M past the reference window (the contig ends)
        mk([(M, 10), (D, 2), (M, 27)], G - 20, ref_len=20),
        mk([(M, 10), (I, 2), (M, 10), (D, 1), (M, 10), (M, 16)], G - 40, ref_len=40),    # the same, more than four operations
        mk([(M, 20), (15, 3), (M, 17)], 600),                           # an unknown operation
        mk([(15, 1)], 700),
        mk([(M, 48)], 800, nbases=40),                                  # an M past the read
        mk([(D, 3)], 900),                                              # a deletion in a read of no bases
        mk([(H, 5), (N, 1)], 1000),
    ]


# ---------------------------------------------------------------- rows of more than 4096 bases
def _bqsr_like_ops(n, rng):
    """About 200 operations, drawn as oracle_bqsr.synth_bqsr_set draws a read's (soft clips at either end, M blocks, short
    insertions and deletions between them), the block lengths scaled to the read."""
    scale = max(1, n // 4100)
    lead = int(rng.integers(1, 8)) if rng.random() < 0.25 else 0
    tail = int(rng.integers(1, 8)) if rng.random() < 0.25 else 0
    blocks, left = [], n - lead - tail
    while left > 0:
        l = int(min(left, rng.integers(8, 40) * scale))
        blocks.append((M, l)); left -= l
        r = rng.random()
        if left > 3 and r < 0.15:
            il = int(rng.integers(1, 4)); blocks.append((I, il)); left -= il
        elif left > 0 and r < 0.3:
            blocks.append((D, int(rng.integers(1, 5))))
    return ([(S, lead)] if lead else []) + blocks + ([(S, tail)] if tail else [])


def long_shapes(n, rng):
    """[(name, ops)] for one row length n > 4096."""
    out = [('one_m', [(M, n)]),
           ('composed_deletion', [(S, 3), (M, 7), (D, 2), (M, n - 10)]),
           ('composed_insertion', [(M, 10), (I, 2), (M, n - 15), (S, 3)])]
    # ONE queued chunk: a deletion too long for its window, its target base t at offset 0, 7, 15 of chunk c -- chunk 0 (the
    # last output chunk of a reverse read), chunk 256 (the first whose index needs a ninth bit) and the last complete one
    for c in sorted({0, 256, (n - 1) // 16 - 1, (n - 1) // 16}):
        for off in (0, 7, 15):
            t = 16 * c + off
            if 3 <= t < n - 1:
                out.append(('queued_%d_%d' % (c, off), [(S, 3), (M, t + 1 - 3), (D, 20), (M, n - t - 1)]))
            elif t == n - 1:
                out.append(('queued_%d_%d' % (c, off), [(S, 3), (M, n - 3), (D, 20), (H, 2)]))
    a = n // 3
    out.append(('five_operations', [(M, a), (I, 2), (M, a), (D, 3), (M, n - 2 * a - 2)]))     # every chunk queued; n >= 32784: the queue overflows
    out.append(('many_operations', _bqsr_like_ops(n, rng)))
    return out


def long_world():
    return World(LONG_GENOME, 20261, runs=4)


def _densify(read, world):
    """Every complete 16-base output chunk with index >= 256 gets at least one expected flag (so that a chunk the kernel never
    wrote cannot pass): where the draw left one empty, one more base of it is substituted."""
    for attempt in range(16):
        e, s = expected(read, world)
        n = len(read)
        full = n // 16
        any_flag = (e | s)[:16 * full].reshape(full, 16).any(1)
        empty = np.flatnonzero(~any_flag)
        empty = empty[empty >= 256]
        if not empty.size:
            return read
        seq = read.seq.copy()
        for j in empty:
            o = 16 * j + attempt                                         # output position -> input position
            i = n - 1 - o if read.is_reverse else o
            seq[i] = ACGT[(np.searchsorted(ACGT, seq[i]) + 1) % 4]
        read = Read(seq, read.cigartuples, read.reference_start, read.reference_end - read.reference_start, read.is_reverse, read.family)
    raise AssertionError('could not give every chunk of %s a flag' % read)


def long_rows(world, n):
    """All shapes of row length n on both strands, placed at random, the first two also at both ends of the genome."""
    rng = np.random.default_rng(8000 + n)
    reads = []
    for k, (name, ops) in enumerate(long_shapes(n, rng)):
        span = ref_span(ops)
        starts = [int(rng.integers(1, world.G - span))] + ([0, world.G - span] if k < 2 else [])
        for st in starts:
            for rev in (False, True):
                reads.append(_densify(build_read(world, ops, st, rev, rng, 'long_%d_%s' % (n, name)), world))
    return reads


def mixed_rows(world):
    """Long and 37-base reads in one batch, under the long pitch."""
    rng = np.random.default_rng(8888)
    reads = long_rows(world, 4113)
    short = [ops for ops in insertion_shapes() + deletion_shapes() + walked_shapes() if read_len(ops) == 37][::9]
    for k, ops in enumerate(short):
        reads.insert((5 * k) % (len(reads) + 1), build_read(world, ops, int(rng.integers(1, world.G - 200)), bool(k & 1), rng, 'mixed_short'))
    return reads


# ---------------------------------------------------------------- K5: the two np.bincount calls over the unskipped bases
def count_q(qual, err, skip, lens, qoffset):
    """(totals[256], errors[256]) of benchmark.calculate_q over the unskipped bases inside the reads."""
    inside = np.arange(qual.shape[1])[None, :] < np.asarray(lens)[:, None]
    counted = inside & (skip == 0)
    q = qual.astype(np.int64) - qoffset
    return (np.bincount(q[counted], minlength=256), np.bincount(q[counted & (err != 0)], minlength=256))


# ---------------------------------------------------------------- K6: reads in sequencing orientation
_COMPLEMENT = np.full(256, ord('N'), dtype=np.uint8)
for _a, _b in zip(b'ACGT', b'TGCA'):
    _COMPLEMENT[_a] = _b


def canonical_reads(seq, oq, err, skip, clip, trim, flags, S, minscore):
    """What K6 writes (kbbq_aligned_kernels.h, the comment above K6Params): per read the aligned part [qs, qe) only, a reverse
    read reverse-complemented (letters outside ACGT -> N), padded with N at quality 0 to the row's end; quality 0 where the base
    is flagged skip, its OQ is below minscore, it lies in the trimmed range or it is N; returns (seq, qual, errmask, meta) with
    errmask = where cseq must differ from seq, meta = S | read group << 16 | read 2 << 31."""
    n, pitch = seq.shape
    out_seq = np.full((n, pitch), ord('N'), dtype=np.uint8)
    out_qual = np.zeros((n, pitch), dtype=np.uint8)
    out_err = np.zeros((n, pitch), dtype=bool)
    for r in range(n):
        qs, qe = int(clip[r]) & 0xFFFF, int(clip[r]) >> 16
        tlo, thi = int(trim[r]) & 0xFFFF, int(trim[r]) >> 16
        pos = np.arange(qs, qe)
        s, q, e = seq[r, qs:qe], oq[r, qs:qe], err[r, qs:qe] != 0
        skipped = (skip[r, qs:qe] != 0) | (q < 33 + minscore) | ((pos >= tlo) & (pos < thi)) | (s == ord('N'))
        q = np.where(skipped, 0, q).astype(np.uint8)
        if int(flags[r]) & 1:
            s, q, e = _COMPLEMENT[s][::-1], q[::-1], e[::-1]
        L = qe - qs
        out_seq[r, :L], out_qual[r, :L], out_err[r, :L] = s, q, e
    fl = np.asarray(flags, dtype=np.uint64)
    meta = (np.uint64(S) | ((fl >> np.uint64(16)) << np.uint64(16)) | (((fl >> np.uint64(1)) & np.uint64(1)) << np.uint64(31))).astype(np.uint32)
    return out_seq, out_qual, out_err, meta


def canonical_cases(L, rng, exhaustive):
    """Rows for K6 at read length L: (clip, trim, flags) -- exhaustive: every (qs, qe) with 0 <= qs < qe <= L on both strands
    without a trimmed range, and again with a trimmed range whose two ends sweep 0..L; otherwise a random sample."""
    clip, trim, flags = [], [], []
    if exhaustive:
        spans = [(a, b) for a in range(L) for b in range(a + 1, L + 1)]
        trims = [(a, b) for a in range(L + 1) for b in range(a, L + 1)]
        k = 0
        for with_trim in (False, True):
            for qs, qe in spans:
                for rev in (0, 1):
                    t = trims[(37 * k) % len(trims)] if with_trim else (0, 0)
                    clip.append(qs | (qe << 16)); trim.append(t[0] | (t[1] << 16))
                    flags.append(rev | ((k >> 1) & 1) << 1 | (k % 3) << 16)
                    k += 1
    else:
        for k in range(48):
            qs = int(rng.integers(0, L // 2)) if k % 4 else 0
            qe = int(rng.integers(max(qs + 1, L // 2), L + 1)) if k % 3 else L
            t = sorted(int(x) for x in rng.integers(0, L + 1, size=2)) if k % 2 else (0, 0)
            clip.append(qs | (qe << 16)); trim.append(t[0] | (t[1] << 16))
            flags.append((k & 1) | ((k >> 1) & 1) << 1 | (k % 3) << 16)
    return np.array(clip, dtype=np.uint32), np.array(trim, dtype=np.uint32), np.array(flags, dtype=np.uint32)


def canonical_inputs(L, seed, exhaustive):
    """Random planes for K6 at read length L: bases with 4 % N (and a few letters outside ACGTN on reverse reads, which become N),
    OQ characters 33..75, flags with bit 0 (error) and bit 1 (skip) each set on a quarter of the bases; 0 behind the read."""
    rng = np.random.default_rng(seed)
    clip, trim, flags = canonical_cases(L, rng, exhaustive)
    n, pitch = len(clip), (L + 15) // 16 * 16
    seq = rng.choice(np.frombuffer(b'ACGTN', dtype=np.uint8), size=(n, pitch), p=[.24, .24, .24, .24, .04])
    odd = (rng.random((n, pitch)) < 0.01) & ((flags & 1) != 0)[:, None]
    seq = np.where(odd, ord('R'), seq).astype(np.uint8)
    oq = rng.integers(33, 33 + 43, size=(n, pitch)).astype(np.uint8)
    err = (rng.random((n, pitch)) < 0.25).astype(np.uint8)
    skip = (rng.random((n, pitch)) < 0.25).astype(np.uint8)
    for a in (seq, oq, err, skip):
        a[:, L:] = 0
    return dict(n=n, pitch=pitch, L=L, seq=seq, oq=oq, err=err, skip=skip, clip=clip, trim=trim, flags=flags,
                len=np.full(n, L, dtype=np.uint32))
