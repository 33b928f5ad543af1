"""
GPU tests (-m gpu) of the aligned-read kernels at every CIGAR boundary and on rows of more than 4096 bases:
K4 (kbbq_find_errors_dev) against oracle_benchmark.find_read_errors, K5 (kbbq_count_q_dev) against np.bincount over the oracle's
unskipped bases, K6 (kbbq_canonical_reads_dev, character and 4-bit planes) against the numpy restatement of its rule, and the
product path gatk.bqsr.bam_to_bqsr_covariates on reads of 4100 bases against oracle_bqsr.  Cases and expected values:
tests/aligned_model.py (what makes them able to fail: tests/test_aligned_model_host.py).

Which path of k4v2_find_errors a family's boundary chunk takes, by the kernel's header (csrc/kbbq_aligned_kernels.h):
  composed from two windows, no walk -- soft clips beside one or between two M ranges; an insertion with both of its M neighbours
      inside the chunk; a deletion / skip behind an M whose sites end inside that base's window (dat + 1 + dlen <= 16, length 0
      included); = and X as M; a soft clip and a short deletion in one chunk (the four-operation shapes);
  queued and walked (k4_walk_chunk) -- an insertion with a neighbour outside the chunk (at the chunk's first or last byte, or 15
      and more bases long); a deletion past its window (dat + 1 + dlen > 16); a deletion and an insertion in one chunk (the order
      shapes); three operations in one chunk; a leading deletion or insertion (Python's index -1); a window that is not wholly
      inside the genome (ref_start = 0 behind a clip, the last genome bytes); every chunk of a read with more than four operations
      (the walked shapes, 2H bM 2P lD restM 3H) and of every shape the reference raises on.
Chunks inside one operation take the plain comparison.
"""
import numpy as np
import pytest

import aligned_model as AM

pytestmark = pytest.mark.gpu

VEC = ['meanq', 'rg_errs', 'rg_total', 'q_errs', 'q_total', 'pos_errs', 'pos_total', 'dinuc_errs', 'dinuc_total']
FILL = 0xA5                                  # what the output planes hold before K4 runs


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from kbbq import _device
    assert 'gfx950' in _device.context().name
    return _device


@pytest.fixture(scope='module')
def OB(oracle):
    import oracle_benchmark
    return oracle_benchmark


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def run_k4(dev, world, arrays, separate_mask, two_planes, flip):
    """One launch of kbbq_find_errors_dev over the CSR arrays -> (err, skip or None) as numpy, the planes pre-filled with FILL."""
    import torch
    from kbbq import _native as N
    n, pitch = arrays['n'], arrays['pitch']
    d = {k: _up(arrays[k]) for k in ('seq', 'len', 'ref_start', 'ref_len', 'cig_off', 'cig_n', 'cigar', 'flip')}
    genome = _up(world.genome if separate_mask else world.fused)
    mask = _up(world.mask) if separate_mask else None
    err = torch.full((n, pitch), FILL, dtype=torch.uint8, device='cuda')
    skip = torch.full((n, pitch), FILL, dtype=torch.uint8, device='cuda') if two_planes else None
    ctx = dev.context()
    N.check(N.load().kbbq_find_errors_dev(ctx.handle, N.ptr(d['seq']), N.ptr(d['len']), n, pitch, N.ptr(d['ref_start']), N.ptr(d['ref_len']),
                                          N.ptr(d['cig_off']), N.ptr(d['cig_n']), N.ptr(d['cigar']), N.ptr(genome), N.ptr(mask), world.G,
                                          N.ptr(d['flip']) if flip else None, N.ptr(err), N.ptr(skip)))
    ctx.status()
    return err.cpu().numpy(), (skip.cpu().numpy() if two_planes else None)


def first_wrong(got, want, where):
    """None, or 'row r chunk j ...' of the first byte inside `where` at which the planes differ."""
    bad = (got != want) & where
    if not bad.any():
        return None
    r, c = (int(x) for x in np.argwhere(bad)[0])
    lo = c // 16 * 16
    return 'row %d chunk %d (byte %d): got %s, expected %s; %d bytes of %d rows wrong' % (
        r, c // 16, c, got[r, lo:lo + 16].tolist(), want[r, lo:lo + 16].tolist(), int(bad.sum()), int(bad.any(1).sum()))


def check_k4(got, reads, world, arrays, flip):
    """Inside a read every byte is the oracle's; from its end to the end of its last chunk the bytes are 0; K4 stores
    ceil(len / 16) chunks of a row, so the chunks behind them still hold FILL."""
    err, skip = got
    we, ws = AM.expected_planes(reads, world, arrays['pitch'], flip)
    stored = np.arange(arrays['pitch'])[None, :] < ((arrays['len'].astype(np.int64) + 15) // 16 * 16)[:, None]
    planes = [('errors', err, we), ('skips', skip, ws)] if skip is not None else [('flags', err, we | (ws << 1))]
    for name, g, w in planes:
        msg = first_wrong(g, w, stored)
        assert msg is None, '%s: %s -- %s' % (name, msg, reads[int(msg.split()[1])])
        msg = first_wrong(g, np.full_like(g, FILL), ~stored)
        assert msg is None, '%s behind the stored chunks: %s -- %s' % (name, msg, reads[int(msg.split()[1])])
    return stored


# ---------------------------------------------------------------- K4, rows of at most 48 bases
@pytest.fixture(scope='module')
def short():
    world = AM.short_world()
    reads = [r for fam in AM.short_families(world).values() for r in fam]
    return world, reads, AM.csr(reads, pitch=64), {}           # pitch 64: every row has a chunk behind its read


CONFIGS = [(m, t, f) for m in (False, True) for t in (True, False) for f in (True, False)]


def _short_k4(dev, short, cfg):
    world, reads, arrays, cache = short
    if cfg not in cache:
        cache[cfg] = run_k4(dev, world, arrays, *cfg)
    return cache[cfg]


@pytest.mark.parametrize('separate_mask,two_planes,flip', CONFIGS)
def test_k4_at_every_boundary_position(dev, short, separate_mask, two_planes, flip):
    world, reads, arrays, _ = short
    assert arrays['seq'].nbytes < 1 << 20
    check_k4(_short_k4(dev, short, (separate_mask, two_planes, flip)), reads, world, arrays, flip)


@pytest.mark.parametrize('separate_mask,two_planes,flip', CONFIGS)
def test_k4_leaves_the_chunks_behind_a_read_alone(dev, short, separate_mask, two_planes, flip):
    """K4 stores ceil(len / 16) chunks of a row: what the planes held in the chunks behind them is still there (check_k4), and
    every row of the short batch has such a chunk."""
    world, reads, arrays, _ = short
    stored = check_k4(_short_k4(dev, short, (separate_mask, two_planes, flip)), reads, world, arrays, flip)
    assert (~stored).any(1).all()


def test_k4_raises_what_the_reference_raises(dev, short):
    """One launch per shape: through compare_reads.find_read_errors, and as a batch of one through the C entry point."""
    from kbbq import aln, compare_reads
    world = short[0]
    ref = {AM.CONTIG: aln.chars(world.genome.tobytes().decode('ascii'))}
    var = {AM.CONTIG: world.mask.astype(bool)}
    reads = AM.raising_reads(world)
    assert len(reads) >= 12
    for r in reads:
        want = AM.expected(r, world)
        assert isinstance(want, type), str(r)
        with pytest.raises(want):
            compare_reads.find_read_errors(r, ref, var)
        with pytest.raises(want):
            run_k4(dev, world, AM.csr([r]), False, False, False)
    # ... and the context is usable afterwards
    ok = AM.build_read(world, [(AM.M, 37)], 100, False, np.random.default_rng(1))
    check_k4(run_k4(dev, world, AM.csr([ok]), False, True, True), [ok], world, AM.csr([ok]), True)


# ---------------------------------------------------------------- K4, rows of more than 4096 bases (more than 256 chunks)
@pytest.fixture(scope='module')
def long_world():
    return AM.long_world()


@pytest.mark.parametrize('n', list(AM.LONG_N) + ['mixed'])
def test_k4_on_rows_over_4096_bases(dev, long_world, n):
    reads = AM.mixed_rows(long_world) if n == 'mixed' else AM.long_rows(long_world, n)
    pitch = AM.pitch_for(reads)
    arrays = AM.csr(reads, pitch=min(pitch + 16, 65536))        # a chunk behind every row, where the pitch can still grow
    assert arrays['pitch'] > 4096
    for separate_mask in (False, True):
        stored = check_k4(run_k4(dev, long_world, arrays, separate_mask, separate_mask, True), reads, long_world, arrays, True)
        assert n == 65535 or (~stored).any(1).all()                      # chunks a wrong chunk index would land in


# ---------------------------------------------------------------- K5 over those planes
def run_k5(dev, qual, err, skip, lens, qoffset):
    import torch
    from kbbq import _native as N
    n, pitch = qual.shape
    counts = torch.zeros(512, dtype=torch.int64, device='cuda')
    d = [_up(qual), _up(err), None if skip is None else _up(skip), _up(lens)]
    ctx = dev.context()
    N.check(N.load().kbbq_count_q_dev(ctx.handle, N.ptr(d[0]), N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]), n, pitch, qoffset, N.ptr(counts)))
    ctx.status()
    h = counts.cpu().numpy()
    return h[:256], h[256:]


def _k5_planes(reads, world, pitch, qoffset, seed):
    """The oracle's flags and a random quality plane (0..93 above the offset); FILL behind every read in all three planes."""
    err, skip = AM.expected_planes(reads, world, pitch)
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    qual = (np.random.default_rng(seed).integers(0, 94, size=err.shape) + qoffset).astype(np.uint8)
    behind = np.arange(pitch)[None, :] >= lens[:, None]
    want = AM.count_q(qual, err, skip, lens, qoffset)
    for a in (err, skip, qual):
        a[behind] = FILL
    return qual, err, skip, lens, want


@pytest.mark.parametrize('qoffset', [0, 33])
@pytest.mark.parametrize('rows', ['short', 'long', 65535])
def test_k5_counts_the_unskipped_bases(dev, short, long_world, rows, qoffset):
    if rows == 'short':
        world, reads, pitch = short[0], short[1], short[2]['pitch']
    else:
        world, reads = long_world, AM.mixed_rows(long_world) if rows == 'long' else AM.long_rows(long_world, 65535)
        pitch = AM.pitch_for(reads)
    qual, err, skip, lens, (total, errors) = _k5_planes(reads, world, pitch, qoffset, 50 + qoffset)
    assert total.sum() > 1000 and errors.sum() > 100 and np.count_nonzero(total) == 94
    for form in ('two planes', 'one plane of flags'):
        flags = (err & 1) | ((skip & 1) << 1)
        flags[np.arange(pitch)[None, :] >= lens[:, None]] = FILL
        t, e = run_k5(dev, qual, err, skip, lens, qoffset) if form == 'two planes' else run_k5(dev, qual, flags, None, lens, qoffset)
        assert np.array_equal(t, total) and np.array_equal(e, errors), form


def test_k5_refuses_a_counted_quality_below_the_offset(dev, short):
    world, reads, arrays, _ = short
    qual, err, skip, lens, _ = _k5_planes(reads[:200], world, arrays['pitch'], 33, 7)
    inside = np.arange(arrays['pitch'])[None, :] < lens[:, None]
    r = int(np.flatnonzero(((skip == 0) & inside).any(1) & ((skip != 0) & inside).any(1))[100])
    c = int(np.flatnonzero(skip[r, :lens[r]] == 0)[0])
    qual[r, c] = 20                                                      # np.bincount of a negative value: ValueError
    with pytest.raises(ValueError):
        run_k5(dev, qual, err, skip, lens, 33)
    qual[r, c] = 33
    skipped = int(np.flatnonzero(skip[r, :lens[r]] != 0)[0])
    qual[r, skipped] = 20                                                # ... a skipped base is never looked at
    t, _ = run_k5(dev, qual, err, skip, lens, 33)
    assert t.sum() == int(((skip == 0) & inside).sum())


# ---------------------------------------------------------------- K6
def run_k6(dev, c, two_planes, nib, minscore):
    """kbbq_canonical_reads_dev (character planes) / kbbq_canonical_reads_rows_dev with KBBQ_ROWS_NIBBLES -> the ReadBatch."""
    from kbbq import _native as N
    n, pitch, L = c['n'], c['pitch'], c['L']
    d = {k: _up(c[k]) for k in ('seq', 'oq', 'len', 'clip', 'trim', 'flags')}
    err = _up(c['err'] if two_planes else c['err'] | (c['skip'] << 1))
    skip = _up(c['skip']) if two_planes else None
    b = dev.ReadBatch(n, pitch, with_corrected=True, nib=nib)
    ctx, lib = dev.context(), N.load()
    common = (ctx.handle, N.ptr(d['seq']), N.ptr(d['oq']), N.ptr(err), N.ptr(skip), N.ptr(d['len']), N.ptr(d['clip']), N.ptr(d['trim']),
              N.ptr(d['flags']), n, pitch, L, minscore, 6)
    outs = (N.ptr(b.seq), N.ptr(b.cseq), N.ptr(b.qual), N.ptr(b.meta))
    if nib:
        N.check(lib.kbbq_canonical_reads_rows_dev(*common, N.ROWS_NIBBLES, *outs))
    else:
        N.check(lib.kbbq_canonical_reads_dev(*common, *outs))
    ctx.status()
    return b


@pytest.mark.parametrize('L,exhaustive,minscore', [(37, True, 6), (37, True, 15), (4100, False, 6)])
def test_k6_writes_the_reads_in_sequencing_orientation(dev, L, exhaustive, minscore):
    """Every aligned part [qs, qe) of a 37-base read on both strands, with and without a trimmed range whose ends sweep the
    read, and a sample on rows of 257 chunks: bases, qualities and sidecar exactly, cseq != seq exactly where an error is flagged."""
    c = AM.canonical_inputs(L, 600 + L, exhaustive)
    if exhaustive:
        assert c['n'] == 2 * 2 * L * (L + 1) // 2
    want_seq, want_qual, want_err, want_meta = AM.canonical_reads(c['seq'], c['oq'], c['err'], c['skip'], c['clip'], c['trim'], c['flags'], L, minscore)
    assert want_err.sum() > c['n'] and (want_qual != 0).sum() > c['n'] and (want_seq[:, :L] == ord('N')).sum() > c['n']
    everywhere = np.ones_like(want_err)
    for two_planes, nib in ((True, False), (False, False), (False, True)):
        b = run_k6(dev, c, two_planes, nib, minscore)
        what = '%s, %s planes' % ('skip plane' if two_planes else 'one plane of flags', '4-bit' if nib else 'character')
        seq, cseq = (b.chars('seq').cpu().numpy(), b.chars('cseq').cpu().numpy()) if nib else (b.seq.cpu().numpy(), b.cseq.cpu().numpy())
        for name, g, w in (('seq', seq, want_seq), ('qual', b.qual.cpu().numpy(), want_qual)):
            msg = first_wrong(g, w, everywhere)
            assert msg is None, '%s %s: %s' % (what, name, msg)
        assert np.array_equal(b.meta.cpu().numpy().view(np.uint32), want_meta), what
        # a corrected N of the 4-bit planes is code 5, which only K1's comparison sees: the characters are compared elsewhere
        where = (want_seq != ord('N')) if nib else everywhere
        msg = first_wrong(cseq != seq, want_err, where)
        assert msg is None, '%s cseq != seq: %s' % (what, msg)


# ---------------------------------------------------------------- K1 on reads whose cycle table is beyond the LDS
@pytest.mark.parametrize('S,lo,R,n,dinuc', [(459, 1, 2, 600, 6), (460, 1, 2, 600, 6), (460, 460, 2, 600, 6), (1001, 1, 2, 600, 6),
                                           (1001, 1001, 2, 600, 6), (460, 1, 2, 600, 20), (1001, 1, 32, 2000, 6)])
def test_k1_counts_every_cycle_of_reads_beyond_its_lds_table(dev, oracle, S, lo, R, n, dinuc):
    """K1 against the oracle's tally where its 43 x (2S | 1) words of cycle counts stop fitting 160 KB of LDS: S = 459 is the
    last shape of one table (163,576 B, k1_accumulate), S = 460 the first in tiles (k1_accumulate_tiled, 2 x 460 cycles), S = 1001
    has 3 tiles of 668 cycles of which the last holds 666.  First and second reads (whose cycles run down from 2 len - 1, so
    lengths 1..S put them in every tile; lo = S puts all of them in the last), every cell of the four tables compared.
    dinuc = 20: the SPLIT instance -- cycles are counted from quality 6, contexts from 20, which is the oracle's context
    tally at minscore 20.  R = 32, n = 2000: 96 workgroups of one CU's LDS each leave 2 per (group, tile) on 256 CUs, the 2000 x
    63 chunks are 247 iterations of 512, so a workgroup runs more than K1_FLUSH_ITERS = 96 and flushes its LDS in between."""
    b = dev.ReadBatch.synthetic(0, n, n, seed=77 + S + lo, len_lo=lo, len_hi=S, nrg=R)
    seq, cseq, qual = (x[:n].cpu().numpy() for x in (b.seq, b.cseq, b.qual))
    meta = b.meta[:n].cpu().numpy().view(np.uint32)
    assert (meta >> 31).sum() > n // 4 and (meta >> 31 == 0).sum() > n // 4 and len(set((meta >> 16) & 0x7FFF)) == R
    want = list(oracle.accumulate(seq, cseq, qual, meta, R, S, minscore=6)[5:9])
    if dinuc != 6:
        every = int(want[3].sum())
        want[2:] = oracle.accumulate(seq, cseq, qual, meta, R, S, minscore=dinuc)[7:9]
        assert 0 < want[3].sum() < every - 1000                    # the second threshold leaves contexts out
    # able to fail: counts and errors in every eighth of the cycle axis (half a tile or less), with reads of one length also in
    # the first and the last 16 cycles, and contexts
    ends = [slice(0, 16), slice(2 * S - 16, 2 * S)] if lo == S else []
    assert all(want[1][:, :, sl].sum() > 1000 and want[0][:, :, sl].sum() > 50
               for sl in [slice(k * S // 4, (k + 1) * S // 4) for k in range(8)] + ends)
    assert want[3].sum() > n and want[2].sum() > 0
    t = dev.Tables(R, 2 * S)
    dev.accumulate(b, t, 6, dinuc_minscore=dinuc)
    for name, got, w in zip(VEC[5:], t.to_host(), want):
        bad = np.argwhere(got != w)
        assert not len(bad), '%s: first wrong (rg, q, column) %s: %d, want %d' % (name, tuple(bad[0]), got[tuple(bad[0])], w[tuple(bad[0])])


# ---------------------------------------------------------------- the product path on rows of 257 chunks
def test_the_tally_of_reads_of_4100_bases(dev, oracle, tmp_path, monkeypatch):
    """gatk.bqsr.bam_to_bqsr_covariates on eight reads of 4100 bases (219..242 operations each) must give the oracle's nine vectors,
    one pass (KBBQ_TALLY_FUSED=2) and K4 -> K6 -> K1 (0).  The one-pass and the fused tally refuse the shape (KBBQ_E_LUT, as
    designed), so both settings end in K4, stand-alone K6 and K1's fallback form with its cycle axis in tiles."""
    import _shim
    import oracle_bqsr as OQ
    from kbbq import aln, benchmark
    from kbbq.gatk import bqsr
    paths = OQ.synth_bqsr_set(str(tmp_path), 4100, npairs=4, S=4100, contigs=(('chr1', 60000),), nrg=2)
    bam = _shim.AlignmentFile(paths['sam'])
    reads = list(bam)
    assert len(reads) == 8 and min(len(r.cigartuples) for r in reads) > 150
    fa = _shim.FastaFile(paths['fa'])
    var = benchmark.get_var_sites(paths['vcf'])
    want = OQ.bam_to_bqsr_covariates(reads, [rg['ID'] for rg in bam.as_dict()['RG']], {c: fa.fetch(c) for c in fa.references}, var)
    assert want[2].sum() > 8 * 4100 // 4
    for fused in ('2', '0'):
        monkeypatch.setenv('KBBQ_TALLY_FUSED', fused)
        got = bqsr.bam_to_bqsr_covariates(aln.AlignmentFile(paths['sam']), paths['fa'], var)
        for k, g, w in zip(VEC, got, want):
            assert np.array_equal(g, w), (k, fused)
