"""
kbbq.benchmark -- truth-set calibration benchmark (reference kbbq/benchmark.py:9-164) with the
per-base work on the MI355X: the CIGAR walk that flags errors and skipped sites
(compare_reads.find_read_errors, K4) and the per-quality counting (calculate_q, K5).
Reference genome, variant sites and confident regions are read from TEXT formats
(kbbq/aln.py); the small per-genome set-up (skip mask) is host NumPy as in the reference.
"""
import numpy as np

from . import aln
from . import compare_reads
from . import fastx
from . import parallel


def get_ref_dict(reffilename):
    """{contig: array of 1-character strings} for every contig of the FASTA."""
    fasta = aln.FastaFile(reffilename)
    return {chrom: aln.chars(fasta.fetch(reference=chrom)) for chrom in fasta.references}


def get_var_sites(vcf):
    """{contig: [0-based positions covered by any record]}."""
    d = dict()
    for record in aln.read_vcf(vcf):
        d.setdefault(record.chrom, list()).extend(range(record.start, record.stop))
    return d


def get_bed_dict(refdict, bedfh):
    beddict = {chrom: np.zeros(len(refdict[chrom]), dtype=bool) for chrom in refdict.keys()}
    for rec in aln.read_bed(bedfh):
        beddict[rec.contig][rec.start:rec.end] = True
    return beddict


def get_full_skips(refdict, var_sites, bedfh=None):
    """Boolean skip mask per contig: variant sites, plus everything outside the BED if given."""
    skips = {chrom: np.zeros(len(refdict[chrom]), dtype=bool) for chrom in refdict.keys()}
    for chrom in skips.keys():
        skips[chrom][np.array(var_sites[chrom], dtype=np.int_)] = True
    if bedfh is not None:
        beddict = get_bed_dict(refdict, bedfh)
        for chrom in skips.keys():
            skips[chrom][~beddict[chrom]] = True
    return skips


def get_bam_readname(read):
    return read.query_name + ("/2" if read.is_read2 else "/1")


def get_fastq_readname(read):
    return read.name.split(sep='_')[0]


# ---------------------------------------------------------------------------
# device batch
# ---------------------------------------------------------------------------
class _Genome:
    """Concatenated contigs + skip mask on the device (uploaded once per benchmark call)."""

    def __init__(self, refdict, fullskips):
        from . import _device as dev
        torch = dev._torch()
        self.offset, parts, masks, pos = {}, [], [], 0
        for chrom, arr in refdict.items():
            self.offset[chrom] = pos
            parts.append(aln.codes(arr)); masks.append(np.asarray(fullskips[chrom], dtype=np.uint8))
            pos += len(arr)
        self.length = pos
        cat = lambda xs: np.concatenate(list(xs)) if xs else np.zeros(0, dtype=np.uint8)
        letters, flags = cat(parts), cat(masks)
        import os
        if os.environ.get('KBBQ_REFERENCE_MASK') != 'separate' and (not len(letters) or int(letters.max()) < 128):
            # ASCII reference: the skip flag rides in bit 7 of every byte (kbbq_find_errors_dev with a NULL mask) --
            # one scattered window per chunk instead of two
            self.genome = torch.from_numpy(np.ascontiguousarray(letters | ((flags != 0).astype(np.uint8) << 7))).cuda()
            self.mask = None
        else:
            self.genome = torch.from_numpy(np.ascontiguousarray(letters)).cuda()
            self.mask = torch.from_numpy(np.ascontiguousarray(flags)).cuda()
        self.sizes = {c: len(a) for c, a in refdict.items()}


def _read_arrays(reads, genome, flip_reverse, rows=None):
    """Host arrays K4 needs, from an aln.AlignmentFile (native reader: vectorised) or from a list of
    pysam-like read objects (one Python pass; the form the reference's own tests use).  rows = (lo, hi): only
    those alignments (one rank's shard); the row pitch is the whole file's, so shards agree on it."""
    if isinstance(reads, aln.AlignmentFile):
        b = reads.batch()
        lo, hi = (0, b.n) if rows is None else rows
        sl = slice(lo, hi)
        n = hi - lo
        lens = b.qlen[sl].astype(np.uint32)
        pitch = fastx.pitch_for(int(b.qlen.max()) if b.n else 1)
        seq = b.plane(0, pitch, lo, n)
        sizes = np.array([genome.sizes[c] for c in b.contig_names] + [0], dtype=np.int64)      # KeyError: unknown contig
        offs = np.array([genome.offset[c] for c in b.contig_names] + [0], dtype=np.int64)
        contig, pos = b.contig[sl], b.pos[sl]
        size = sizes[contig] if n else np.zeros(0, np.int64)
        start = np.minimum(np.maximum(pos, 0), size)                 # Python slice clamping of the reference window
        end = np.minimum(np.maximum(pos + b.ref_span[sl], start), size)
        ref_start = (offs[contig] if n else np.zeros(0, np.int64)) + start
        ref_len = (end - start).astype(np.int32)
        flip = ((b.flag[sl] & 16) != 0).astype(np.uint8) if flip_reverse else np.zeros(n, dtype=np.uint8)
        return n, lens, pitch, seq, ref_start, ref_len, b.cig_off[sl], b.cig_n[sl], b.cigar, flip   # offsets into the whole CIGAR array
    longest = max([len(r.query_sequence) for r in reads] + [1])
    if rows is not None:
        reads = reads[rows[0]:rows[1]]
    n = len(reads)
    lens = np.array([len(r.query_sequence) for r in reads], dtype=np.uint32)
    pitch = fastx.pitch_for(longest)
    seq = np.zeros((max(n, 1), pitch), dtype=np.uint8)
    ref_start = np.zeros(n, dtype=np.int64); ref_len = np.zeros(n, dtype=np.int32)
    cig_off = np.zeros(n, dtype=np.uint32); cig_n = np.zeros(n, dtype=np.uint32)
    flip = np.zeros(n, dtype=np.uint8)
    cigar = []
    for i, r in enumerate(reads):
        seq[i, :lens[i]] = aln.codes(r.query_sequence)
        size = genome.sizes[r.reference_name]                      # KeyError: unknown contig, as in the reference
        start = min(max(r.reference_start, 0), size)               # Python slice clamping of the reference window
        end = min(max(r.reference_end, start), size)
        ref_start[i] = genome.offset[r.reference_name] + start
        ref_len[i] = end - start
        cig_off[i] = len(cigar); cig_n[i] = len(r.cigartuples)
        for op, l in r.cigartuples:
            code = op if isinstance(op, (int, np.integer)) and 0 <= op <= 8 else 15   # 15: unrecognised -> ValueError
            cigar.append((int(l) << 4) | int(code))
        flip[i] = 1 if (flip_reverse and r.is_reverse) else 0
    return n, lens, pitch, seq, ref_start, ref_len, cig_off, cig_n, np.array(cigar, dtype=np.uint32), flip


def _upload_reads(reads, genome, flip_reverse, rows=None):
    """The arrays K4 reads, on the device: dict(n, lens (host), pitch, seq, len, cigar, ref_start, ref_len, flip, cig_off, cig_n)
    of an aln.AlignmentFile or a list of read objects; rows = (lo, hi): only those alignments (one rank's shard)."""
    from . import _device as dev
    torch = dev._torch()
    n, lens, pitch, seq, ref_start, ref_len, cig_off, cig_n, cigar, flip = _read_arrays(reads, genome, flip_reverse, rows)
    pad = lambda a, dt: np.ascontiguousarray(a if len(a) else np.zeros(1), dtype=dt)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(n=n, lens=lens, pitch=pitch, seq=up(seq), len=up(pad(lens, np.uint32).view(np.int32)),
                cigar=up(pad(cigar, np.uint32).view(np.int32)), ref_start=up(pad(ref_start, np.int64)),
                ref_len=up(pad(ref_len, np.int32)), flip=up(pad(flip, np.uint8)),
                cig_off=up(pad(cig_off, np.uint32).view(np.int32)), cig_n=up(pad(cig_n, np.uint32).view(np.int32)))


def _find_errors(u, genome, fused=False):
    """K4 over uploaded reads (_upload_reads) -> (err, skip) device planes [n, pitch]; fused: ONE plane of flags (bit 0 error,
    bit 1 skip) comes back as `err` and `skip` is None -- the form K5 / K6 read when they are the only consumers."""
    from . import _device as dev
    from . import _native as N
    torch = dev._torch()
    n, pitch = u['n'], u['pitch']
    err = torch.zeros((max(n, 1), pitch), dtype=torch.uint8, device='cuda')
    skip = None if fused else torch.zeros((max(n, 1), pitch), dtype=torch.uint8, device='cuda')
    ctx = dev.context()
    N.check(N.load().kbbq_find_errors_dev(ctx.handle, N.ptr(u['seq']), N.ptr(u['len']), n, pitch,
                                          N.ptr(u['ref_start']), N.ptr(u['ref_len']), N.ptr(u['cig_off']), N.ptr(u['cig_n']),
                                          N.ptr(u['cigar']), N.ptr(genome.genome), N.ptr(genome.mask), genome.length,
                                          N.ptr(u['flip']), N.ptr(err), N.ptr(skip)))
    ctx.status()
    return err, skip


def _flag_batch(reads, genome, flip_reverse, keep=None, rows=None, fused=False):
    """K4 over aligned reads (an aln.AlignmentFile or a list of read objects) -> (err, skip) device planes
    [n, pitch], lens (host).  `keep`, a dict, receives the device seq plane for callers that go on to K6.
    rows = (lo, hi): only those alignments (one rank's shard).  fused: see _find_errors."""
    u = _upload_reads(reads, genome, flip_reverse, rows)
    if keep is not None:
        keep['seq'] = u['seq']
    err, skip = _find_errors(u, genome, fused)
    return err, skip, u['lens'], u['pitch']


def _match_native(bam, fq):
    """Row of the alignment for every FASTQ read (benchmark.py:102-124), matched in C++."""
    from . import _native as N
    n = fq.n
    idx = np.zeros(max(n, 1), dtype=np.int64)
    N.check(N.load().kbbq_sam_match_fastq(bam.batch()._handle.h, fq._h, N.ptr(idx)))
    idx = idx[:n]
    if n and int(idx.min()) < 0:
        raise KeyError(fq.name(int(np.flatnonzero(idx < 0)[0])).split('_')[0])
    return idx


def _bam_names(reads):
    """Canonical read names (benchmark.py:41-48): QNAME + /1 or /2."""
    if isinstance(reads, aln.AlignmentFile):
        b = reads.batch()
        second = (b.flag & 128) != 0
        return [nm + ('/2' if s else '/1') for nm, s in zip(b.names(), second)]
    return [get_bam_readname(r) for r in reads]


def _count_q(qual, err, skip, lens, pitch, qoffset, reduce=False):
    """K5 -> (numerrs[256], numtotal[256]) as int64 host arrays; reduce: summed over all ranks."""
    from . import _device as dev
    from . import _native as N
    torch = dev._torch()
    n = len(lens)
    counts = torch.zeros(512, dtype=torch.int64, device='cuda')
    d_len = torch.from_numpy(np.ascontiguousarray(lens.astype(np.uint32)).view(np.int32)).cuda() if n else torch.zeros(1, dtype=torch.int32, device='cuda')
    ctx = dev.context()
    N.check(N.load().kbbq_count_q_dev(ctx.handle, N.ptr(qual), N.ptr(err), N.ptr(skip), N.ptr(d_len),
                                      n, pitch, qoffset, N.ptr(counts)))
    ctx.status()
    if reduce:
        parallel.allreduce_tables(counts)                        # one 4 KB sum over the ranks' shards
    h = counts.cpu().numpy()
    return h[256:].copy(), h[:256].copy()


def _actual_q(numerrs, numtotal):
    """benchmark.py:83-91 from the two count vectors (trimmed to the largest observed quality)."""
    top = np.flatnonzero(numtotal)
    size = int(top[-1]) + 1 if top.size else 0
    numtotal, numerrs = numtotal[:size], numerrs[:size]
    nonzero = numtotal != 0
    q = compare_reads.p_to_q(np.true_divide(numerrs[nonzero], numtotal[nonzero]))
    actual_q = np.zeros(len(numtotal), dtype=np.int_)
    actual_q[nonzero] = q
    return actual_q, numtotal.astype(np.int_)


def get_error_dict(bamfile, refdict, fullskips):
    """{canonical read name: (errors, skips)} -- flags of reverse-strand reads flipped, because a
    FASTQ made from the BAM holds them reverse-complemented."""
    reads = bamfile if isinstance(bamfile, aln.AlignmentFile) else list(bamfile)
    genome = _Genome(refdict, fullskips)
    err, skip, lens, _ = _flag_batch(reads, genome, flip_reverse=True)
    e, s = err.cpu().numpy().astype(bool), skip.cpu().numpy().astype(bool)
    return {name: (e[i, :lens[i]].copy(), s[i, :lens[i]].copy()) for i, name in enumerate(_bam_names(reads))}


def calculate_q(errors, quals):
    """(actual_q, numtotal) indexed by predicted quality, from flat arrays (reference
    benchmark.py:76-91).  The two bincounts run on the device (K5)."""
    from . import _device as dev
    torch = dev._torch()
    errors = np.asarray(errors, dtype=bool).reshape(-1)
    quals = np.asarray(quals).reshape(-1)
    if quals.size and (quals.min() < 0 or quals.max() > 255):
        raise ValueError('qualities must lie in 0..255')
    n = quals.size
    pitch = fastx.pitch_for(max(n, 1))
    if pitch > 65536:                      # long flat input: fold into rows of 4096
        pitch = 4096
    rows = max(1, -(-n // pitch))
    q = np.zeros(rows * pitch, dtype=np.uint8); q[:n] = quals
    e = np.zeros(rows * pitch, dtype=np.uint8); e[:n] = errors
    lens = np.full(rows, pitch, dtype=np.uint32); lens[-1] = n - (rows - 1) * pitch
    up = lambda a: torch.from_numpy(a.reshape(rows, pitch)).cuda()
    d_q, d_e = up(q), up(e)
    d_s = torch.zeros((rows, pitch), dtype=torch.uint8, device='cuda')
    numerrs, numtotal = _count_q(d_q, d_e, d_s, lens, pitch, 0)
    return _actual_q(numerrs, numtotal)


def get_bamread_quals(read, use_oq=False):
    if use_oq:
        return np.array([ord(c) - 33 for c in read.get_tag('OQ')], dtype=np.int_)
    return np.array(read.query_qualities, dtype=np.int_)


def _qual_plane(reads, lens, pitch, use_oq, rows=None):
    """uint8 plane of phred values (not characters) per read (of alignments rows = (lo, hi) only)."""
    if isinstance(reads, aln.AlignmentFile):
        b = reads.batch()
        lo, hi = (0, b.n) if rows is None else rows
        n = hi - lo
        have = (b.oq_len if use_oq else b.qual_len)[lo:hi]
        if use_oq and n and int(have.min()) < 0:
            raise KeyError("tag 'OQ' not present")
        if n and np.any(have != lens):
            i = int(np.flatnonzero(have != lens)[0])
            raise _at(IndexError('boolean index did not match indexed array: read %d has %d qualities for %d bases'
                                 % (lo + i, int(have[i]), int(lens[i]))), i)
        chars = b.plane(2 if use_oq else 1, pitch, lo, n)
        inside = np.arange(pitch)[None, :] < np.asarray(lens)[:, None] if n else np.zeros((1, pitch), dtype=bool)
        if n and int(chars[:n][inside].min(initial=255)) < 33:
            raise ValueError('qualities must lie in 0..255')
        return np.where(inside, chars[:max(n, 1)] - 33, 0).astype(np.uint8)
    if rows is not None:
        reads = reads[rows[0]:rows[1]]
    q = np.zeros((max(len(reads), 1), pitch), dtype=np.uint8)
    for i, r in enumerate(reads):
        v = get_bamread_quals(r, use_oq)
        if len(v) != lens[i]:
            raise IndexError('boolean index did not match indexed array: read %d has %d qualities for %d bases'
                             % (i, len(v), lens[i]))
        if v.size and (v.min() < 0 or v.max() > 255):
            raise ValueError('qualities must lie in 0..255')
        q[i, :lens[i]] = v
    return q


def _qual_chars_dev(reads, lens, pitch, use_oq, rows=None):
    """The quality characters (QUAL, or the OQ tag) of a native reader's alignments as a device plane [n, pitch], zero behind every
    read -- checked like _qual_plane: lengths on the host arrays, the value range on the device (every byte below '!' must be padding)."""
    from . import _device as dev
    torch = dev._torch()
    b = reads.batch()
    lo, hi = (0, b.n) if rows is None else rows
    n = hi - lo
    have = (b.oq_len if use_oq else b.qual_len)[lo:hi]
    if use_oq and n and int(have.min()) < 0:
        raise KeyError("tag 'OQ' not present")
    if n and np.any(have != lens):
        i = int(np.flatnonzero(have != lens)[0])
        raise _at(IndexError('boolean index did not match indexed array: read %d has %d qualities for %d bases'
                             % (lo + i, int(have[i]), int(lens[i]))), i)
    chars = torch.from_numpy(b.plane(2 if use_oq else 1, pitch, lo, n)).cuda()
    if n and int((chars[:n] < 33).sum().item()) != n * pitch - int(np.asarray(lens, dtype=np.int64).sum()):
        raise ValueError('qualities must lie in 0..255')
    return chars


def _at(exc, index):
    """Tag an exception with the read of this rank's shard it is about (as the kernels' status does): the ranks then
    agree on the first one (parallel.raise_first_error)."""
    exc.read_index = int(index)
    return exc


def _on_all_ranks(fn, first=0):
    """fn() on this rank's shard; an exception of any rank's data is raised by every rank (the one of the smallest
    read index), so that nobody is left waiting in the sum of the counts."""
    exc, res = None, None
    try:
        res = fn()
    except (IndexError, TypeError, ValueError, KeyError) as e:
        exc = e
    parallel.raise_first_error(exc, None if exc is None else first + max(getattr(exc, 'read_index', 0), 0))
    return res


def benchmark_bam(bamfile, ref, var_sites, use_oq=False, bedfh=None):
    """Under torch.distributed (parallel.init_from_env) every rank flags and counts a contiguous shard of the
    alignments; the per-quality counts are summed with one allreduce (SURVEY 8(e) applied to this path)."""
    from . import _device as dev
    torch = dev._torch()
    fullskips = get_full_skips(ref, var_sites, bedfh)
    reads = bamfile if isinstance(bamfile, aln.AlignmentFile) else list(bamfile)
    world, rank = parallel.world_rank()
    rows = parallel.shard_range(len(reads), rank, world) if world > 1 else None
    genome = _Genome(ref, fullskips)

    def shard():
        err, skip, lens, pitch = _flag_batch(reads, genome, flip_reverse=False, rows=rows, fused=True)
        if isinstance(reads, aln.AlignmentFile):
            # the native reader's plane of quality CHARACTERS goes up as it is and K5 subtracts the 33 (three masked NumPy passes over
            # the plane were 60 % of this function: 47 ms per 200 K alignments); a character below '!' is the reference's ValueError
            qual, offset = _qual_chars_dev(reads, lens, pitch, use_oq, rows), 33
        else:
            qual, offset = torch.from_numpy(_qual_plane(reads, lens, pitch, use_oq, rows)).cuda(), 0
        return qual, err, skip, lens, pitch, offset
    qual, err, skip, lens, pitch, offset = _on_all_ranks(shard, rows[0] if rows else 0)
    return _actual_q(*_count_q(qual, err, skip, lens, pitch, offset, reduce=world > 1))


LAST_RUN = {}            # what the most recent benchmark_fastq flagged on this rank (tests, KBBQ_TIMING): K4's share of the alignments


def benchmark_fastq(fqfile, bamfile, ref, var_sites, bedfh=None):
    """Under torch.distributed every rank counts a contiguous shard of the FASTQ reads and flags (K4) ONLY the
    alignments its reads map to: the name join of the reference (benchmark.py:93-104) is one host pass every rank makes
    over the names -- no flags, no bases -- and tells the rank the span of alignment rows [first, last] its shard needs
    (a FASTQ made from the BAM keeps its order: about 1 / world of the rows); K4 runs over that span, K5 over the shard,
    and the 512 per-quality counters are summed with one allreduce."""
    from . import _device as dev
    import sys
    torch = dev._torch()
    fullskips = get_full_skips(ref, var_sites, bedfh)
    reads = bamfile if isinstance(bamfile, aln.AlignmentFile) else list(bamfile)
    fq = fastx.NativeFastq(fqfile)
    if isinstance(reads, aln.AlignmentFile):
        idx = _match_native(reads, fq)                               # both sides native: no Python object per read
    else:
        row = {}
        for i, name in enumerate(_bam_names(reads)):
            row[name] = i                                            # later reads replace earlier ones (dict)
        idx = np.array([row[fq.name(i).split('_')[0]] for i in range(fq.n)], dtype=np.int64)   # KeyError if absent
    n, S, _, kind, bad = fq.scan(None, False)
    world, rank = parallel.world_rank()
    lo, hi = parallel.shard_range(fq.n, rank, world) if world > 1 else (0, fq.n)
    m = hi - lo
    idx = idx[lo:hi]
    nalign = reads.batch().n if isinstance(reads, aln.AlignmentFile) else len(reads)
    # the rows K4 walks on this rank: what its FASTQ reads map to, and its own contiguous share of the alignments (so that the
    # ranks together look at EVERY alignment, as get_error_dict does -- bad input is reported whoever's reads map to it)
    a_lo, a_hi = parallel.shard_range(nalign, rank, world) if world > 1 else (0, nalign)
    if m:
        a_lo, a_hi = min(a_lo, int(idx.min())), max(a_hi, int(idx.max()) + 1)
    genome = _Genome(ref, fullskips)

    def flag_shard():
        return _flag_batch(reads, genome, flip_reverse=True, fused=True, rows=(a_lo, a_hi))
    err, skip, lens, pitch = _on_all_ranks(flag_shard, a_lo)
    LAST_RUN.clear()
    LAST_RUN.update(rank=rank, world=world, fastq_reads=m, alignments=nalign, k4_alignments=a_hi - a_lo)
    from . import _trace
    if _trace.ON:
        sys.stderr.write('kbbq benchmark: rank %d of %d counts FASTQ reads [%d, %d) and flagged alignments [%d, %d): %d of %d\n'
                         % (rank, world, lo, hi, a_lo, a_hi, a_hi - a_lo, nalign))
    idx = idx - a_lo
    _, _, fqual, fmeta = fq.fill(None, False, m, max(pitch, fastx.pitch_for(S)), first=lo)
    flens = (fmeta & 0xFFFF).astype(np.uint32)

    def check():
        if np.any(flens != lens[idx]):
            raise _at(IndexError('boolean index did not match indexed array: FASTQ and BAM read lengths differ'),
                      int(np.flatnonzero(flens != lens[idx])[0]))
    _on_all_ranks(check, lo)
    d_idx = torch.from_numpy(np.ascontiguousarray(idx)).cuda()
    fp = fqual.shape[1]
    e = torch.zeros((max(m, 1), fp), dtype=torch.uint8, device='cuda')          # the flags of every FASTQ read's alignment
    if m:
        e[:m, :pitch] = err.index_select(0, d_idx)
    return _actual_q(*_count_q(torch.from_numpy(fqual).cuda(), e, None, flens, fp, 33, reduce=world > 1))


def print_benchmark(actual_q, label, nbases):
    """Tab-separated rows: predicted quality, actual quality, label, number of bases."""
    nonzero = (nbases != 0)
    for pq, aq, nb in zip(np.arange(len(actual_q))[nonzero], actual_q[nonzero], nbases[nonzero]):
        print(pq, aq, label, nb, sep="\t")


# ---------------------------------------------------------------------------
# benchmark --kmers: the k-mer rule's flags against the truth set's
# ---------------------------------------------------------------------------
CONFUSION_BASES_PER_LAUNCH = (1 << 32) - 1     # KBBQ_CONFUSION_MAX_BASES: what one kbbq_flag_confusion_dev call takes (nreads * pitch)

KMER_COLUMNS = ('#predicted_q', 'bases', 'errors', 'flagged', 'flagged_errors', 'unresolved', 'unresolved_errors', 'actual_q',
                'kmer_q', 'kmer_q_skip', 'label')


def kmer_confusion(qual, truth, kflags, lens, pitch, qoffset):
    """The joint tally of K4's one plane of flags (`truth`: bit 0 error, bit 1 skip) and the k-mer rule's plane (`kflags`:
    kbbq.kmer.flag_errors(unresolved=True): 0 trusted, 1 error, 2 unresolved) by quality: an int64 host array
    joint[q][truth error][k-mer class] of shape (256, 2, 3) over the bases inside their reads whose skip bit is clear
    (kbbq_flag_confusion_dev).  qual / truth / kflags: device planes [n, pitch] of the same rows; lens: host array.  The rows
    go in launches of at most CONFUSION_BASES_PER_LAUNCH bases (the kernel's counters are 32 bits wide), which all add into
    the same device counters.  A counted base whose quality byte is below qoffset: ValueError with its read."""
    from . import _device as dev
    from . import _native as N
    torch = dev._torch()
    n = len(lens)
    counts = torch.zeros(256 * 2 * 3, dtype=torch.int64, device='cuda')
    if n:
        d_len = torch.from_numpy(np.ascontiguousarray(np.asarray(lens).astype(np.uint32)).view(np.int32)).cuda()
        step = max(1, int(CONFUSION_BASES_PER_LAUNCH) // int(pitch))
        ctx = dev.context()
        lib = N.load()
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            N.check(lib.kbbq_flag_confusion_dev(ctx.handle, N.ptr(qual[lo:hi]), N.ptr(truth[lo:hi]), N.ptr(kflags[lo:hi]),
                                                N.ptr(d_len[lo:hi]), hi - lo, pitch, qoffset, N.ptr(counts)))
            try:
                ctx.status()
            except ValueError as exc:
                i = getattr(exc, 'read_index', -1)
                if lo == 0 or i < 0:
                    raise
                raise _at(ValueError('read %d: a counted base has a quality byte below the offset %d (row %d of the launch that '
                                     'began at read %d)' % (lo + i, qoffset, i, lo)), lo + i) from None
    return counts.cpu().numpy().reshape(256, 2, 3).copy()


def _kmer_benchmark_inputs(bamfile, k, min_count, prefilter, filter_bits):
    """Everything benchmark_kmers refuses on its arguments, before any device call and, in a process group, before any
    collective (as gatk.bqsr._kmer_inputs)."""
    from . import kmer
    if kmer._ranks() is not None:
        raise ValueError('benchmark --kmers does not run across ranks yet: the k-mer table of the alignments is counted and '
                         'read on one GPU; run `kbbq benchmark` without --kmers under ranks, or with --kmers on one GPU')
    if not 8 <= int(k) <= 32:
        raise ValueError('k must be in 8..32, got %d' % int(k))
    if min_count is not None and int(min_count) < 1:
        raise ValueError('min_count must be >= 1, got %d' % int(min_count))
    if prefilter:
        kmer._check_prefilter(min_count, filter_bits)
    if not isinstance(bamfile, aln.AlignmentFile):
        raise TypeError('benchmark_kmers takes a kbbq.aln.AlignmentFile (its batch() arrays), got %s' % type(bamfile).__name__)
    return bamfile.batch()


def benchmark_kmers(bamfile, ref, var_sites, k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, use_oq=False,
                    bedfh=None, info=None, passes=1, partitions=1, kmer_min_qual=None, kmers_from=None):
    """How good is the k-mer rule on a truth set?  joint[q][truth error][k-mer class], int64 (256, 2, 3): every base of the
    alignments that benchmark_bam counts (not at a variant site, inside the BED, not soft-clipped), by its reported quality
    (QUAL, or the OQ tag with use_oq), by whether it differs from the reference (K4, exactly as benchmark_bam flags it) and
    by what the k-mers of the alignments' own sequences say about it: 0 trusted, 1 error, 2 unresolved (untrusted, and no
    substitution wins) -- the decisions `kbbq bqsr --kmers [--skip-unresolved]` tallies.
    The k-mers are counted from the SEQ plane uploaded for K4: every base of every record, soft clips included, canonical
    keys; then as gatk.bqsr.bam_to_kmer_covariates: optional prefilter, a table of default_slots within the device budget less
    the four resident planes (or `slots`), the count histogram's first valley unless min_count is given, flag_errors with
    unresolved bases.  Records may have any lengths (a record shorter than k has no k-mer: all its bases are class 0).
    One GPU; bamfile is a kbbq.aln.AlignmentFile.  `info`, a dict, receives k, min_count, reads, slots, prefilter, admitted,
    bases, errors, flagged, flagged_errors, unresolved and unresolved_errors (totals over the counted bases).
    passes: the classes of `passes` passes of the rule (flag_errors(passes=...): 1 where the last pass ends on another letter,
    2 where the base is unchanged and its row's last evaluation left it unresolved); `info` then receives passes too.
    partitions: as gatk.bqsr.bam_to_kmer_covariates' -- the count in that many rounds (kmer.count_block), the classes read
    from the solid table: the same joint array; with more than one round `info` receives partitions, kept_pairs and solid_slots.
    kmer_min_qual = Q (kmer.gate_plane): only the k-mers whose bases all have quality >= Q -- the plane the confusion reads -- are
    counted; the prefilter, the count and every partition round read the gated copy of SEQ, which sizes the filter and the
    default table, and the classes are decided for SEQ as read.  A record with bases and without qualities (QUAL '*', or no OQ
    tag with use_oq) is refused with a ValueError naming it, before any upload.  `info` then receives kmer_min_qual,
    counted_windows and windows.
    kmers_from = PATH (kmer.load_set): the classes are read from the table of a k-mer set file -- the very set `bqsr --kmers
    --kmers-from` decided by -- instead of a count of these alignments; k is the set's (pass k=None, or the set's), no counting
    option goes with it; `info` then receives kmers_from and loaded_kmers, and its slots is the loaded table's."""
    from . import _device as dev
    from . import kmer
    passes = kmer.check_passes(passes)
    kmers_from = kmer.check_kmers_from(kmers_from, prefilter, filter_bits, partitions, kmer_min_qual)
    if kmers_from is not None:
        k = kmer.set_k(kmers_from, k)                # the header alone: no device
    partitions = kmer._check_partitions(partitions)
    kmer_min_qual = kmer.check_kmer_min_qual(kmer_min_qual)
    b = _kmer_benchmark_inputs(bamfile, k, min_count, prefilter, filter_bits)
    if kmer_min_qual is not None and b.n:
        have = b.oq_len if use_oq else b.qual_len
        bare = np.flatnonzero((have <= 0) & (b.qlen > 0))
        if bare.size:
            i = int(bare[0])
            raise ValueError('record %d (%s) has no %s: benchmark --kmers --kmer-min-qual needs a quality for every base'
                             % (i, b._text(0, i), 'OQ tag' if use_oq else "qualities (QUAL '*')"))
    k = int(k)
    torch = dev._torch()
    fullskips = get_full_skips(ref, var_sites, bedfh)
    genome = _Genome(ref, fullskips)
    keep = {}
    truth, _, lens, pitch = _flag_batch(bamfile, genome, flip_reverse=False, keep=keep, fused=True)
    qual = _qual_chars_dev(bamfile, lens, pitch, use_oq)
    n = len(lens)
    t, counting = (int(min_count) if min_count is not None else 0), dict(slots=0, admitted=None)   # of a file without records
    if n:
        d_seq = keep['seq']
        d_len = torch.from_numpy(np.ascontiguousarray(lens.astype(np.uint32)).view(np.int32)).cuda()
        budget = dev.device_budget()
        resident = 4 * n * pitch + 20 * n           # SEQ, qualities, the truth flags and the k-mer flags; the per-read words
        windows = ungated = kmer.kmer_total(lens, k)
        counted = d_seq                             # the plane the prefilter and the count read
        if kmer_min_qual is not None:
            counted, windows = kmer.gate_plane(d_seq, qual, d_len, k, kmer_min_qual)
            resident += n * pitch                   # ... until the count is over

        def read(what, **kw):
            (kmer.prefilter_kmers if what == 'prefilter' else kmer.count_kmers)(counted, d_len, k=k, **kw)
        table = None
        try:
            table, _, t, counting = kmer.count_block(read, windows, k, min_count=min_count, slots=slots, prefilter=prefilter,
                                                     filter_bits=filter_bits, partitions=partitions, kmers_from=kmers_from,
                                                     room=budget - resident)
            del counted
            kflags, _, _ = kmer.flag_errors(table, d_seq, d_len, t, unresolved=True, **kmer._passes_kw(passes))
        finally:
            if table is not None:
                table.close()
        joint = kmer_confusion(qual, truth, kflags, lens, pitch, 33)
    else:
        joint = np.zeros((256, 2, 3), dtype=np.int64)
    if info is not None:
        info.update(k=k, min_count=t, reads=n, slots=counting['slots'], prefilter=bool(prefilter), admitted=counting['admitted'],
                    **kmer_totals(joint))
        if passes != 1:
            info.update(passes=passes)
        if counting.get('partitions', 1) > 1:
            info.update({key: counting[key] for key in ('partitions', 'kept_pairs', 'solid_slots')})
        if kmer_min_qual is not None:
            info.update(kmer_min_qual=kmer_min_qual, counted_windows=windows if n else 0, windows=ungated if n else 0)
        if kmers_from is not None:
            info.update(kmers_from=kmers_from, loaded_kmers=counting.get('loaded_kmers', 0))
    return joint


def kmer_totals(joint):
    """The totals of a joint array over all qualities: bases, errors, flagged, flagged_errors, unresolved, unresolved_errors."""
    J = np.asarray(joint).sum(axis=0)
    return dict(bases=int(J.sum()), errors=int(J[1].sum()), flagged=int(J[:, 1].sum()), flagged_errors=int(J[1, 1]),
                unresolved=int(J[:, 2].sum()), unresolved_errors=int(J[1, 2]))


def kmer_summary(info):
    """The one line `kbbq benchmark --kmers` writes to stderr (without the newline); a ratio whose denominator is 0 prints 0.0000."""
    ratio = lambda a, b: (a / b) if b else 0.0
    line = ('kbbq benchmark: k=%d min_count=%d reads=%d bases=%d errors=%d flagged=%d flagged_errors=%d unresolved=%d '
            'unresolved_errors=%d precision=%.4f recall=%.4f'
            % (info['k'], info['min_count'], info['reads'], info['bases'], info['errors'], info['flagged'], info['flagged_errors'],
               info['unresolved'], info['unresolved_errors'], ratio(info['flagged_errors'], info['flagged']),
               ratio(info['flagged_errors'], info['errors'])))
    if info.get('passes', 1) > 1:
        line += ' passes=%d' % info['passes']
    if info.get('partitions', 1) > 1:
        line += ' partitions=%d' % info['partitions']
    if info.get('kmer_min_qual') is not None:
        line += ' kmer_min_qual=%d counted_windows=%d' % (info['kmer_min_qual'], info['counted_windows'])
    if info.get('prefilter'):
        line += ' prefilter=1 admitted=%d slots=%d' % (info['admitted'], info['slots'])
    if info.get('kmers_from'):
        line += ' kmers_from=1 loaded_kmers=%d' % info['loaded_kmers']
    return line


def print_benchmark_kmers(joint, label):
    """A header line, then one tab-separated row per quality with bases != 0, ascending.  With J = joint[q]: bases J.sum(),
    errors J[1].sum(), flagged J[:, 1].sum(), flagged_errors J[1, 1], unresolved J[:, 2].sum(), unresolved_errors J[1, 2];
    actual_q = p_to_q(errors / bases), what `benchmark` prints; kmer_q = p_to_q(flagged / bases), the quality `bqsr --kmers`
    tallies; kmer_q_skip = p_to_q(flagged / (bases - unresolved)), 0 where that denominator is 0, what `--skip-unresolved`
    tallies."""
    joint = np.asarray(joint)
    print(*KMER_COLUMNS, sep='\t')
    for q in np.flatnonzero(joint.sum(axis=(1, 2))):
        J = joint[q]
        bases, errors, flagged, unresolved = int(J.sum()), int(J[1].sum()), int(J[:, 1].sum()), int(J[:, 2].sum())
        p_to_q = lambda a, b: int(compare_reads.p_to_q(np.true_divide(a, b)))
        print(int(q), bases, errors, flagged, int(J[1, 1]), unresolved, int(J[1, 2]), p_to_q(errors, bases), p_to_q(flagged, bases),
              p_to_q(flagged, bases - unresolved) if bases != unresolved else 0, label, sep='\t')


def benchmark(bamfile, fafile, vcffile, fastqfile=None, label=None, use_oq=False, bedfh=None, kmers=None):
    """Run the benchmark and print it.  With a FASTQ, its reads are matched to the alignments by name.  kmers: a dict of
    benchmark_kmers' options (k, min_count, slots, prefilter, filter_bits, passes, partitions, kmer_min_qual, kmers_from) -- print the k-mer rule's flags against the truth
    set's instead (print_benchmark_kmers) and one summary line on stderr."""
    if kmers is not None and fastqfile is not None:
        raise ValueError('benchmark --kmers takes the alignments alone (-b), not a FASTQ joined by name (-f)')
    bam = aln.AlignmentFile(bamfile, 'r')
    ref = get_ref_dict(fafile)
    var_sites = get_var_sites(vcffile)
    if kmers is not None:
        import sys
        info = {}
        joint = benchmark_kmers(bam, ref, var_sites, use_oq=use_oq, bedfh=bedfh, info=info, **kmers)
        print_benchmark_kmers(joint, bamfile if label is None else label)
        sys.stdout.flush()
        sys.stderr.write(kmer_summary(info) + '\n')
        return
    if fastqfile is not None:
        actual_q, nbases = benchmark_fastq(fastqfile, bam, ref, var_sites, bedfh)
        label = (fastqfile if label is None else label)
    else:
        actual_q, nbases = benchmark_bam(bam, ref, var_sites, use_oq, bedfh)
        label = (bamfile if label is None else label)
    if parallel.world_rank()[1] == 0:                                # every rank holds the same totals
        print_benchmark(actual_q, label, nbases)
