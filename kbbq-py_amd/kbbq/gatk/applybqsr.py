"""
kbbq.gatk.applybqsr -- get_delta_qs is on the hot path (reference
kbbq/gatk/applybqsr.py:80-103); table_to_vectors (:14-44) turns a stored GATK report back
into the nine model vectors.  The per-read ApplyBQSR emulation on
aligned reads (:46-78) is host NumPy, one read at a time, as in the reference (it has no batch
caller there; reads come from kbbq.aln or pysam).  recalibrate_alignments is the batch form on the GPU (every alignment of
an aln.AlignmentFile through kbbq_apply_aligned: csrc/kbbq_apply_aligned.h) and apply_report the report -> SAM flow of the
`kbbq applybqsr` command.
"""
import numpy as np

from .. import _bgzf
from .. import compare_reads as utils


def table_to_vectors(table, rg_order, maxscore=42):
    """RecalibrationReport -> (meanq, global_errs, global_total, q_errs, q_total, pos_errs,
    pos_total, dinuc_errs, dinuc_total) for the read groups of rg_order, in that order
    (reference applybqsr.py:14-44).  Cells the report does not list are zero; the cycle axis is
    2 x the largest cycle number present, laid out 1..n then -n..-1; meanq is the report's
    EstimatedQReported (float64).  A read group missing from RecalTable0 cannot be cast to
    integer counts in the reference either (NaN): ValueError."""
    rg_order = list(rg_order)
    rg_index = {str(name): i for i, name in enumerate(rg_order)}
    R, Q = len(rg_order), maxscore + 1

    t0 = table.tables[2].data
    rows0 = {str(name): pos for pos, name in enumerate(t0.index)}
    missing = [name for name in rg_index if name not in rows0]
    if missing:
        raise ValueError('Cannot convert non-finite values (NA or inf) to integer: read group %r is not in the report'
                         % missing[0])
    pick = np.array([rows0[str(name)] for name in rg_order], dtype=np.int64)
    meanq = t0['EstimatedQReported'].to_numpy()[pick].astype(np.float64)
    global_errs = t0['Errors'].to_numpy()[pick].astype(np.int64)
    global_total = t0['Observations'].to_numpy()[pick]

    def scatter(shape, idx, values):
        out = np.zeros(shape, dtype=np.int64)
        out[idx] = np.asarray(values).astype(np.int64)
        return out

    t1 = table.tables[3].data
    rg1 = np.array([rg_index.get(str(x), -1) for x in t1.index.get_level_values('ReadGroup')], dtype=np.int64)
    q1 = t1.index.get_level_values('QualityScore').to_numpy().astype(np.int64)
    ok = (rg1 >= 0) & (q1 >= 0) & (q1 < Q)
    q_errs = scatter((R, Q), (rg1[ok], q1[ok]), t1['Errors'].to_numpy()[ok])
    q_total = scatter((R, Q), (rg1[ok], q1[ok]), t1['Observations'].to_numpy()[ok])

    t2 = table.tables[4].data
    rg2 = np.array([rg_index.get(str(x), -1) for x in t2.index.get_level_values('ReadGroup')], dtype=np.int64)
    q2 = t2.index.get_level_values('QualityScore').to_numpy().astype(np.int64)
    name2 = t2.index.get_level_values('CovariateName').to_numpy().astype(str)
    value2 = t2.index.get_level_values('CovariateValue').to_numpy().astype(str)
    errs2, obs2 = t2['Errors'].to_numpy(), t2['Observations'].to_numpy()
    inside = (rg2 >= 0) & (q2 >= 0) & (q2 < Q)

    cyc = inside & (name2 == 'Cycle')
    if not cyc.any():
        raise ValueError('cannot convert float NaN to integer: the report lists no Cycle rows for these read groups')
    cycles = value2[cyc].astype(np.int64)
    seqlen = int(cycles.max())
    # 1..n -> columns 0..n-1; -n..-1 -> columns n..2n-1; anything else is not on the reindexed grid
    col = np.where(cycles > 0, cycles - 1, 2 * seqlen + cycles)
    on_grid = (cycles != 0) & (cycles >= -seqlen)
    idx = (rg2[cyc][on_grid], q2[cyc][on_grid], col[on_grid])
    pos_errs = scatter((R, Q, 2 * seqlen), idx, errs2[cyc][on_grid])
    pos_total = scatter((R, Q, 2 * seqlen), idx, obs2[cyc][on_grid])

    ctx = inside & (name2 == 'Context')
    code = np.array([utils.Dinucleotide.dinuc_to_int.get(v, -1) for v in value2[ctx]], dtype=np.int64)
    known = code >= 0
    idx = (rg2[ctx][known], q2[ctx][known], code[known])
    dinuc_errs = scatter((R, Q, 16), idx, errs2[ctx][known])
    dinuc_total = scatter((R, Q, 16), idx, obs2[ctx][known])

    return meanq, global_errs, global_total, q_errs, q_total, pos_errs, pos_total, dinuc_errs, dinuc_total


def get_delta_qs(meanq, rg_errs, rg_total, q_errs, q_total, pos_errs, pos_total,
                 dinuc_errs, dinuc_total):
    """Hierarchical delta-Q solve: read group, then reported quality given the read
    group, then cycle and dinucleotide given both.  Returns
    (rgdeltaq[R], qscoredeltaq[R,Q], positiondeltaq[R,Q,2S], dinucdeltaq[R,Q,17]);
    the 17th dinucleotide column is zero so that context -1 adds nothing."""
    meanq = np.asarray(meanq)
    rg_dq = utils.gatk_delta_q(meanq, rg_errs, rg_total)
    level1 = np.broadcast_to((meanq + rg_dq)[:, np.newaxis], np.shape(q_total)).copy()
    q_dq = utils.gatk_delta_q(level1, q_errs, q_total)
    level2 = level1 + q_dq
    pos_dq = utils.gatk_delta_q(np.broadcast_to(level2[..., np.newaxis], np.shape(pos_total)).copy(),
                                pos_errs, pos_total)
    dn_dq = utils.gatk_delta_q(np.broadcast_to(level2[..., np.newaxis], np.shape(dinuc_total)).copy(),
                               dinuc_errs, dinuc_total)
    dn_dq = np.concatenate([dn_dq, np.zeros(dn_dq.shape[:-1] + (1,), dtype=dn_dq.dtype)], axis=-1)
    return rg_dq.copy(), q_dq.copy(), pos_dq.copy(), dn_dq.copy()


def _oriented_quals(read, use_oq):
    return utils.bamread_get_oq(read) if use_oq else np.array(read.query_qualities, dtype=np.int_)


def bamread_cycle_covariates(read):
    """Cycle of every base in ALIGNED order: 0..L-1 (first in pair) or -1..-L (second), reversed for a
    reverse-strand read (reference applybqsr.py:46-50)."""
    cycle = utils.generic_cycle_covariate(read.query_length, read.is_read2)
    return np.flip(cycle) if read.is_reverse else cycle


def bamread_dinuc_covariates(read, use_oq=True, minscore=6):
    """Dinucleotide context of every base in aligned order, computed in sequencing orientation (reverse-strand reads
    reverse-complemented, unknown letters -> N) and flipped back (reference applybqsr.py:52-63)."""
    seq, quals = read.query_sequence, _oriented_quals(read, use_oq)
    if read.is_reverse:
        seq = ''.join(utils.Dinucleotide.complement.get(x, 'N') for x in reversed(seq))
        quals = np.flip(quals)
    dinuc = utils.generic_dinuc_covariate(np.array(list(seq), dtype='U1'), quals, minscore)
    return np.flip(dinuc) if read.is_reverse else dinuc


def recalibrate_bamread(read, meanq, globaldeltaq, qscoredeltaq, positiondeltaq, dinucdeltaq, rg_to_int, use_oq=True,
                        minscore=6):
    """New qualities of one aligned read (reference applybqsr.py:65-78): bases at or above minscore get
    meanq + the four deltas of their read group / quality / context / cycle, the others keep their quality.
    As in the reference the context is always taken from the OQ tag's qualities with minscore 6."""
    original = _oriented_quals(read, use_oq)
    out = np.array(original, dtype=np.int_)
    rg = rg_to_int[read.get_tag('RG')]
    valid = original >= minscore
    q = original[valid]
    cycle = bamread_cycle_covariates(read)[valid]
    dinuc = bamread_dinuc_covariates(read)[valid]
    out[valid] = (meanq[rg] + globaldeltaq[rg] + qscoredeltaq[rg, q] + dinucdeltaq[rg, q, dinuc]
                  + positiondeltaq[rg, q, cycle]).astype(np.int_)
    return out



# ---- the batch path: every alignment of a file on the GPU -------------------------------------------------------------------

LAST_RUN = {}                  # what the last recalibrate_alignments / write_alignments call did: model form, alignments
_ROWS = 1 << 20                # alignments per host slab (planes of SEQ / QUAL / OQ / output)
_MAX_RG = 4096                 # read groups the kernel's row word holds


def quantize_map(levels, round_down=False, minscore=6):
    """The byte map of --static-quantized-quals (include/kbbq_hip.h, "Static quantized qualities") as np.uint8[256].
    levels: a non-empty collection of integers minscore <= Q <= 93; E = sorted({minscore} U levels).  An output byte b below
    33 + minscore maps to itself; q = b - 33 at or above E[-1] to E[-1] + 33; E[i] <= q < E[i + 1] to the nearer of the two,
    ties down -- with round_down always to E[i].  ValueError for empty levels, a level that is not an integer, or one out of
    range."""
    import numbers
    minscore = int(minscore)
    try:
        levels = list(levels)
    except TypeError:
        raise ValueError('quantization levels must be a collection of integers, got %r' % (levels,)) from None
    if not levels:
        raise ValueError('static quantized qualities need at least one level')
    for q in levels:
        if isinstance(q, bool) or not isinstance(q, numbers.Integral):
            raise ValueError('quantization level %r is not an integer' % (q,))
        if not minscore <= q <= 93:
            raise ValueError('quantization level %d is outside %d..93' % (q, minscore))
    E = np.array(sorted({minscore} | {int(q) for q in levels}), dtype=np.int64)
    q = np.arange(256, dtype=np.int64) - 33
    lo = E[np.clip(np.searchsorted(E, q, side='right') - 1, 0, len(E) - 1)]
    hi = E[np.clip(np.searchsorted(E, q, side='right'), 0, len(E) - 1)]          # (== lo at and above the top level)
    new = lo if round_down else np.where(2 * q <= lo + hi, lo, hi)
    return (np.where(q < minscore, q, new) + 33).astype(np.uint8)


def _check_qmap(quantize):
    """quantize=None, or the 256-byte map (quantize_map) as a contiguous np.uint8 array."""
    if quantize is None:
        return None
    qmap = np.ascontiguousarray(quantize)
    if qmap.dtype != np.uint8 or qmap.shape != (256,):
        raise ValueError('quantize: the 256-byte map of quantize_map (np.uint8[256])')
    return qmap


def _model(meanq, rgdq, qdq, posdq, dndq, minscore):
    """The five model arrays -> (mode, host blob, R, Qt, S2) for kbbq_apply_aligned.  An integer model is kbbq_build_lut's blob,
    as the FASTQ path uses it.  A float model (a report's EstimatedQReported, float deltas) is folded into the same integer rows
    only when that is proven exact: for every (rg, q, context, cycle) cell, trunc((base + dinuc) + pos) -- the reference's float64
    sum, base = meanq + rgdq + qdq -- must equal cycle entry + context entry.  Otherwise the kernel sums the float64 rows itself."""
    from .. import _native as N
    meanq, rgdq, qdq, posdq, dndq = (np.asarray(x) for x in (meanq, rgdq, qdq, posdq, dndq))
    R, Qt = qdq.shape
    S2, D = posdq.shape[2], dndq.shape[2]
    if D not in (16, 17) or meanq.shape != (R,) or rgdq.shape != (R,) or posdq.shape[:2] != (R, Qt) or dndq.shape[:2] != (R, Qt):
        raise ValueError('model arrays of inconsistent shapes')
    if R > _MAX_RG:
        raise ValueError('at most %d read groups' % _MAX_RG)
    if D == 16:                                                  # index -1 aliases the last column, as in the reference
        dndq = np.concatenate([dndq, dndq[..., 15:16]], axis=-1)
    lib = N.load()
    integer = all(x.dtype.kind in 'iub' for x in (meanq, rgdq, qdq, posdq, dndq))
    if integer and Qt <= 95:
        blob = np.zeros((lib.kbbq_lut_bytes(R, Qt, S2) + 15) // 16 * 16, dtype=np.uint8)
        args = [np.ascontiguousarray(x, dtype=np.int64) for x in (meanq, rgdq, qdq, posdq, dndq)]
        flags = __import__('ctypes').c_int(0)
        rc = lib.kbbq_build_lut(R, Qt, S2, 17, minscore, *[N.ptr(a) for a in args], N.ptr(blob), __import__('ctypes').byref(flags))
        if rc == N.KBBQ_OK:
            return N.ALIGNED_LUT, blob, R, Qt, S2
        if rc != N.KBBQ_E_RANGE:                                 # (an entry beyond int16: the float64 rows below hold it exactly)
            N.check(rc)
    base = meanq[:, None] + rgdq[:, None] + qdq                 # [R, Qt], summed as the reference sums it
    dn = dndq.astype(np.result_type(base, dndq))
    if not integer and Qt <= 95:
        rs = lib.kbbq_lut_row_stride(S2)
        lut = np.zeros((R, Qt, rs), dtype=np.int16)
        exact = True
        for r in range(R):
            full = np.trunc((base[r][:, None, None] + dn[r][:, :, None]) + posdq[r][:, None, :])      # [Qt, 17, S2]
            cyc = full[:, 16, :]
            ctx = full[:, :, 0] - cyc[:, :1]
            if (not np.array_equal(full, cyc[:, None, :] + ctx[:, :, None]) or np.abs(cyc).max() > 32767
                    or np.abs(ctx).max() > 32767):
                exact = False
                break
            lut[r, :, :S2] = cyc
            five = np.full((Qt, 5, 5), 16)
            five[:, :4, :4] = np.arange(16).reshape(4, 4)
            lut[r, :, S2:S2 + 25] = np.take_along_axis(ctx, five.reshape(Qt, 25), axis=1)
        if exact:
            return N.ALIGNED_LUT, lut.view(np.uint8).reshape(-1), R, Qt, S2
    if Qt > 223:
        raise ValueError('at most 223 quality levels')
    rows = np.concatenate([base[..., None].astype(np.float64), dn.astype(np.float64), posdq.astype(np.float64)], axis=-1)
    return N.ALIGNED_F64, np.ascontiguousarray(rows).view(np.uint8).reshape(-1), R, Qt, S2


def _rows(bam, rg_to_int, R, use_oq, lo, hi):
    """Row words and bookkeeping of alignments [lo, hi) (include/kbbq_hip.h, kbbq_apply_aligned).  A record whose source
    qualities are '*' or absent passes through (length 0 here; its QUAL as read goes out); a record without an OQ tag takes
    its context from the source plane.  KeyError for a recalibrated record whose RG is missing or unknown, ValueError for one
    whose SEQ, QUAL and OQ lengths disagree -- each with .read_index."""
    b = bam.batch()
    sl = slice(lo, hi)
    L = b.qlen[sl].astype(np.int64)
    qual_len, oq_len = b.qual_len[sl].astype(np.int64), b.oq_len[sl].astype(np.int64)
    has_oq = oq_len >= 0
    src_len = oq_len if use_oq else qual_len
    passthrough = (~has_oq) if use_oq else (qual_len == 0)
    passthrough |= L == 0
    names = b.rg_ids
    model_rg = np.array([rg_to_int.get(x, -1) for x in names] + [-1, -1], dtype=np.int64)      # [-2] / [-1]: unknown / missing
    rg = model_rg[b.rg[sl]]
    bad_rg = ~passthrough & (rg < 0)
    if (~passthrough & (rg >= R)).any():
        k = int(np.flatnonzero(~passthrough & (rg >= R))[0])
        exc = IndexError('index %d is out of bounds for axis 0 with size %d' % (int(rg[k]), R))
        exc.read_index = lo + k
        raise exc
    bad_len = ~passthrough & ((src_len != L) | (has_oq & (oq_len != L)))
    first_bad = min([int(np.flatnonzero(x)[0]) for x in (bad_rg, bad_len) if x.any()] or [hi - lo])
    if first_bad < hi - lo:                                  # (the error, and how many records before it can still run)
        k = first_bad
        if bad_len[k]:
            exc = ValueError('alignment %d: SEQ, QUAL and OQ lengths differ' % (lo + k))
        else:
            tag = b.rg[lo + k]
            exc = KeyError("tag 'RG' not present" if tag == -1 else names[tag] if tag >= 0
                           else b.line(lo + k).split('RG:Z:')[1].split('\t')[0])
        exc.read_index = lo + k
        return k, exc
    flag = b.flag[sl].astype(np.uint32)
    meta = (np.where(passthrough, 0, L).astype(np.uint32) | (np.maximum(rg, 0).astype(np.uint32) << 16)
            | (np.uint32(1 << 28) if use_oq else np.uint32(0)) | (has_oq.astype(np.uint32) << 29)
            | (((flag & 16) != 0).astype(np.uint32) << 30) | (((flag & 128) != 0).astype(np.uint32) << 31))
    return meta, passthrough


def _recalibrated_slabs(bam, model, rg_to_int, use_oq, minscore, lo, hi, quantize=None):
    """(first alignment, count, output plane [count, pitch] of QUAL characters, lengths) for slabs of alignments [lo, hi): the
    kernel's new qualities + 33, pass-through records holding their QUAL as read.  quantize: the 256-byte map the new
    qualities go through in the kernel (kbbq_apply_aligned_q); pass-through records are not touched."""
    import ctypes
    from .. import _device as dev
    from .. import _native as N
    mode, blob, R, Qt, S2 = model
    b = bam.batch()
    pitch = max(16, (int(b.maxlen) + 15) // 16 * 16)
    ctx = None
    for first in range(lo, hi, _ROWS):
        m = min(_ROWS, hi - first)
        rows = _rows(bam, rg_to_int, R, use_oq, first, first + m)
        stop = None
        if isinstance(rows[1], Exception):                   # a record the reference would reject: the ones before it still run
            k, stop = rows
            if k > 0:
                rows = _rows(bam, rg_to_int, R, use_oq, first, first + k)
            m = k
        if m > 0:
            meta, passthrough = rows
            seq = b.plane(0, pitch, first, m)
            has_oq = bool((b.oq_len[first:first + m] >= 0).any())
            oq = b.plane(2, pitch, first, m) if (use_oq or has_oq) else None
            qual = b.plane(1, pitch, first, m) if (not use_oq or passthrough.any()) else None
            out = np.empty((m, pitch), dtype=np.uint8)
            if ctx is None:
                ctx = dev.context()
            bad = ctypes.c_int64(-1)
            args = (ctx.handle, N.ptr(seq), N.ptr(qual if not use_oq else oq), N.ptr(oq), N.ptr(meta),
                    m, pitch, R, Qt, S2, minscore, N.ptr(blob), blob.nbytes, mode, N.ptr(out), ctypes.byref(bad))
            if quantize is None:
                rc = N.load().kbbq_apply_aligned(*args)
            else:
                rc = N.load().kbbq_apply_aligned_q(*args, N.ptr(quantize))
            try:
                N.check(rc)
            except Exception as exc:
                exc.read_index = first + int(bad.value) if bad.value >= 0 else first
                raise
            if passthrough.any():
                out[passthrough] = qual[passthrough]
            lens = np.where(passthrough, b.qual_len[first:first + m], b.qlen[first:first + m]).astype(np.int64)
            yield first, m, out, lens
        if stop is not None:
            raise stop


def _resident_slabs(bam, model, rg_to_int, use_oq, minscore, lo, hi, resident, quantize=None, device=False):
    """_recalibrated_slabs for alignments whose planes are on the device already (`resident`: gatk.bqsr._kmer_tally's -- seq and
    source [n, pitch], and oq, the context plane, where records carry OQ tags and the source is QUAL): the same slabs, row
    words, pass-through, errors and error order; kbbq_apply_aligned_dev reads the planes where they lie and only the output
    plane of a slab crosses the bus.  quantize: as _recalibrated_slabs (kbbq_apply_aligned_q_dev).
    device: the output plane stays where the kernel wrote it -- (first, count, device output plane, None, the slab's rows of the
    device SEQ plane, pass-through mask); a pass-through record's row of the plane is not its QUAL (write_alignments_bam)."""
    from .. import _device as dev
    from .. import _native as N
    mode, blob, R, Qt, S2 = model
    b = bam.batch()
    pitch = resident['pitch']
    if pitch != max(16, (int(b.maxlen) + 15) // 16 * 16):
        raise ValueError('resident planes of pitch %d for alignments of up to %d bases' % (pitch, int(b.maxlen)))
    T = dev._torch()
    d_seq, d_src, d_oq = resident['seq'], resident['source'], resident.get('oq')
    ctx = d_blob = d_qmap = None
    for first in range(lo, hi, _ROWS):
        m = min(_ROWS, hi - first)
        rows = _rows(bam, rg_to_int, R, use_oq, first, first + m)
        stop = None
        if isinstance(rows[1], Exception):                   # a record the reference would reject: the ones before it still run
            k, stop = rows
            if k > 0:
                rows = _rows(bam, rg_to_int, R, use_oq, first, first + k)
            m = k
        if m > 0:
            meta, passthrough = rows
            has_oq = bool((b.oq_len[first:first + m] >= 0).any())
            if ctx is None:
                ctx = dev.context()
                d_blob = T.from_numpy(blob).cuda()
                d_qmap = None if quantize is None else T.from_numpy(quantize).cuda()
            d_meta = T.from_numpy(np.ascontiguousarray(meta).view(np.int32)).cuda()
            d_out = T.empty((m, pitch), dtype=T.uint8, device='cuda')
            ctx_plane = d_src if use_oq or not has_oq else d_oq
            args = (ctx.handle, N.ptr(d_seq[first:first + m]), N.ptr(d_src[first:first + m]), N.ptr(ctx_plane[first:first + m]),
                    N.ptr(d_meta), m, pitch, R, Qt, S2, minscore, N.ptr(d_blob), mode, N.ptr(d_out))
            if d_qmap is None:
                N.check(N.load().kbbq_apply_aligned_dev(*args))
            else:
                N.check(N.load().kbbq_apply_aligned_q_dev(*args, N.ptr(d_qmap)))
            try:
                ctx.status()
            except Exception as exc:
                exc.read_index = first + max(getattr(exc, 'read_index', 0), 0)
                raise
            if device:
                yield first, m, d_out, None, d_seq[first:first + m], passthrough
                if stop is not None:
                    raise stop
                continue
            out = d_out.cpu().numpy()
            if passthrough.any():
                out[passthrough] = b.plane(1, pitch, first, m)[passthrough]
            lens = np.where(passthrough, b.qual_len[first:first + m], b.qlen[first:first + m]).astype(np.int64)
            yield first, m, out, lens
        if stop is not None:
            raise stop


class _Window:
    """Rows [first, first + len) of a whole-file plane on the device, sliced by the file's row numbers as _resident_slabs does."""

    def __init__(self, rows, first):
        self.rows, self.first = rows, first

    def __getitem__(self, key):
        return self.rows[key.start - self.first:key.stop - self.first]


def _uploaded_slabs(bam, model, rg_to_int, use_oq, minscore, lo, hi, quantize=None):
    """_resident_slabs(device=True) for alignments whose planes are not on the device: the planes kbbq_apply_aligned would stage
    go up slab by slab -- the same bytes -- and stay there with the output plane, for the BAM assemble kernel to read."""
    from .. import _device as dev
    T = dev._torch()
    b = bam.batch()
    pitch = max(16, (int(b.maxlen) + 15) // 16 * 16)
    for first in range(lo, hi, _ROWS):
        m = min(_ROWS, hi - first)
        up = lambda which: _Window(T.from_numpy(b.plane(which, pitch, first, m)).cuda(), first)     # noqa: E731
        resident = dict(pitch=pitch, seq=up(0), source=up(2 if use_oq else 1))
        if not use_oq and bool((b.oq_len[first:first + m] >= 0).any()):
            resident['oq'] = up(2)
        yield from _resident_slabs(bam, model, rg_to_int, use_oq, minscore, first, first + m, resident, quantize, device=True)


def device_resident(bam, use_oq):
    """_resident_slabs' planes of an aln.DeviceAlignments: where the decode left them."""
    b = bam.batch()
    resident = dict(pitch=b.pitch, seq=b.device_plane(0, b.pitch), source=b.device_plane(2 if use_oq else 1, b.pitch))
    if not use_oq and bool((b.oq_len >= 0).any()):
        resident['oq'] = b.device_plane(2, b.pitch)
    return resident


def recalibrate_alignments(bam, meanq, rgdq, qdq, posdq, dndq, rg_to_int, use_oq=True, minscore=6, quantize=None):
    """New qualities of every alignment of an aln.AlignmentFile (SAM or BAM) on the GPU (kbbq_apply_aligned), as one flat int
    array and offsets [n + 1]: alignment i's are quals[offsets[i]:offsets[i + 1]], equal to recalibrate_bamread(read_i, ...)
    for every read the reference can process.  The same exceptions as the per-read function (IndexError, TypeError, KeyError),
    for the first offending alignment, with .read_index.  Beyond the reference: a record without an OQ tag takes its context from
    the source qualities (the reference: KeyError), and one whose source qualities are '*' or absent is passed through (its QUAL as
    read).  New qualities outside -33..222 cannot be written as SAM: ValueError, as on the FASTQ path.
    quantize: the 256-byte map of quantize_map; every new quality goes through it after the errors above have been decided."""
    quantize = _check_qmap(quantize)
    model = _model(meanq, rgdq, qdq, posdq, dndq, minscore)
    quals, lens = [], []
    n = len(bam)
    for first, m, out, ln in _recalibrated_slabs(bam, model, rg_to_int, use_oq, minscore, 0, n, quantize):
        quals.append(out[np.arange(out.shape[1]) < ln[:, None]].astype(np.int_) - 33)
        lens.append(ln)
    LAST_RUN.clear()
    LAST_RUN.update(mode='lut' if model[0] == 0 else 'f64', alignments=n)
    lens = np.concatenate(lens) if lens else np.zeros(0, np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return (np.concatenate(quals) if quals else np.zeros(0, np.int_)), offsets


def write_alignments(bam, meanq, rgdq, qdq, posdq, dndq, rg_to_int, sink, use_oq=False, set_oq=False, minscore=6,
                     rows=None, header=True, resident=None, quantize=None):
    """Recalibrated SAM text of alignments rows = (lo, hi) (all by default) to the binary file `sink`: the header lines as read
    (header=True), then every alignment line as read with its QUAL replaced and, with set_oq, an OQ tag holding the QUAL as
    read added where there is none (csrc/sam_host.cpp kbbq_sam_render).  resident: the alignments' planes where they are on the
    device already (_resident_slabs), instead of filled and uploaded slab by slab.  quantize: the 256-byte map of quantize_map
    for the new QUAL; the OQ tag of set_oq holds the qualities as read."""
    import ctypes
    from .. import _native as N
    from .._egress import _Reserve
    quantize = _check_qmap(quantize)
    lib = N.load()
    b = bam.batch()
    lo, hi = (0, len(bam)) if rows is None else rows
    model = _model(meanq, rgdq, qdq, posdq, dndq, minscore)
    reserve = _Reserve(sink)
    if header:
        text = ''.join(line + '\n' for line in bam.header).encode('latin-1')
        reserve.ahead(len(text))
        sink.write(text)
    slabs = (_recalibrated_slabs(bam, model, rg_to_int, use_oq, minscore, lo, hi, quantize) if resident is None else
             _resident_slabs(bam, model, rg_to_int, use_oq, minscore, lo, hi, resident, quantize))
    for first, m, out, _ in slabs:
        need = ctypes.c_size_t(0)
        N.check(lib.kbbq_sam_render(b._native, first, m, N.ptr(out), out.shape[1], int(bool(set_oq)), None, 0, ctypes.byref(need)))
        buf = np.empty(max(need.value, 1), dtype=np.uint8)
        N.check(lib.kbbq_sam_render(b._native, first, m, N.ptr(out), out.shape[1], int(bool(set_oq)), N.ptr(buf), buf.nbytes,
                                    ctypes.byref(need)))
        reserve.ahead(need.value)
        sink.write(memoryview(buf)[:need.value])
    LAST_RUN.clear()
    LAST_RUN.update(mode='lut' if model[0] == 0 else 'f64', alignments=hi - lo)


def write_alignments_bam(bam, meanq, rgdq, qdq, posdq, dndq, rg_to_int, writer, use_oq=False, set_oq=False, minscore=6,
                         rows=None, header=True, resident=None, quantize=None):
    """write_alignments as a BAM stream into a kbbq._bamout.BamWriter: the stream is the one the SAM text of write_alignments
    defines (include/kbbq_hip.h "BAM output").  The output plane of the apply and the SEQ plane it read stay on the device
    (_resident_slabs / _uploaded_slabs, device=True) and the writer's assemble kernel reads them there; what goes up beyond the
    apply's own planes is the records' skeleton and descriptors, what comes back is compressed blocks.  The records must have
    passed kbbq._bamout.check."""
    quantize = _check_qmap(quantize)
    lo, hi = (0, len(bam)) if rows is None else rows
    model = _model(meanq, rgdq, qdq, posdq, dndq, minscore)
    if header:
        writer.header(bam)
    slabs = (_uploaded_slabs(bam, model, rg_to_int, use_oq, minscore, lo, hi, quantize) if resident is None else
             _resident_slabs(bam, model, rg_to_int, use_oq, minscore, lo, hi, resident, quantize, device=True))
    for first, m, d_out, _, d_seq, passthrough in slabs:
        writer.records(bam.batch(), first, m, set_oq, passthrough, d_seq, d_out, int(d_out.shape[1]))
    LAST_RUN.clear()
    LAST_RUN.update(mode='lut' if model[0] == 0 else 'f64', alignments=hi - lo)


def check_bam_index(bam, output, index):
    """What --bam-index refuses of a parsed file, before the output exists: no file name (an index of stdout has no name), a
    reference too long for `bai`, alignments out of coordinate order or beyond the index's reach (kbbq._bamindex)."""
    from .. import _bamindex
    if output is None:
        raise ValueError('--bam-index needs -o FILE: the index is written beside it (FILE.bai / FILE.csi)')
    _, depth = _bamindex.resolve(index, bam.header)
    _bamindex.check(bam, depth)


def write_bam_file(bam, output, write, index=None):
    """The BAM file of a command: kbbq._bamout.check (ValueError before the file exists), then write(writer) into a BamWriter
    over `output`, or over stdout for None.  LAST_RUN['bam_out']: the closed writer's counters.  index (--bam-index: auto, bai,
    csi): check_bam_index, then the file's index beside it, made in the same pass; its counters join the others."""
    from .. import _bamout
    _bamout.check(bam)
    if index is not None:
        check_bam_index(bam, output, index)
    with (_bamout.stdout_sink() if output is None else _bamout.open_sink(output, **({} if index is None else {'index': index}))) as writer:
        write(writer)
    LAST_RUN['bam_out'] = {key: getattr(writer, key) for key in ('h2d_bytes', 'd2h_bytes', 'stream_bytes', 'file_bytes')
                           + (() if index is None else ('index_bytes', 'index_runs', 'index_d2h_bytes'))}


def check_bam_index_options(bam_index, bam_out, output):
    """What --bam-index refuses of its command's options."""
    from .. import _bamindex
    if bam_index not in _bamindex.KINDS:
        raise ValueError('--bam-index: one of %s, got %r' % (', '.join(_bamindex.KINDS), bam_index))
    if not bam_out:
        raise ValueError('--bam-index: only with --bam-out (it indexes the BAM file that option writes)')
    if output is None:
        raise ValueError('--bam-index needs -o FILE: the index is written beside it (FILE.bai / FILE.csi)')


BAM_OUT_RANKS = ('--bam-out does not run across ranks in this version (one BAM file is one stream of blocks): on one GPU, or '
                 'without the option -- the SAM text path runs under ranks, every rank writing OUTPUT.rankNNNN')


def report_model(bam, report_path):
    """A stored GATK report -> (meanq, rgdq, qdq, posdq, dndq, rg_to_int) for the read groups of bam's header (reference
    tests/test_gatk_applybqsr.py:123-134: the report names read groups by their PU)."""
    from .. import recaltable
    return _report_model(bam, recaltable.RecalibrationReport.fromfile(report_path))


def _report_model(bam, report):
    """report_model of a report that has been parsed (from a file, or from the text one would hold: RecalibrationReport.fromtext)."""
    rg_to_pu = utils.get_rg_to_pu(bam)
    rg_to_int = {r: i for i, r in enumerate(rg_to_pu)}
    meanq, *vectors = table_to_vectors(report, list(rg_to_pu.values()))
    return (meanq,) + tuple(get_delta_qs(meanq, *vectors)) + (rg_to_int,)


@_bgzf.option
def apply_report(bam, report_path, use_oq=False, set_oq=False, output=None, quantize=None, bam_out=False, bam_index=None):
    """`kbbq applybqsr`: report -> model (table_to_vectors, get_delta_qs on the device) -> kbbq_apply_aligned -> SAM text, to
    `output` or stdout.  Under torch.distributed.run every rank takes parallel.shard_range of the alignments and writes
    output.rankNNNN, the header in rank 0's file only, so that the files concatenated in rank order are the single-process
    output.  Without bam_out an output name ending in .bam is refused.  quantize: the 256-byte map of quantize_map
    (--static-quantized-quals); per byte, so the rank files concatenated stay the one-process bytes.
    bam_out (--bam-out): the same records as a BAM file, whatever its name (write_alignments_bam); one process only, not with
    bgzf; what BAM cannot hold is a ValueError before the file is created (kbbq._bamout.check).
    bam_index (--bam-index: auto, bai or csi): with bam_out and an output name, the file's BAI / CSI index beside it, reduced on
    the GPU in the same pass (kbbq/_bamindex.py); the alignments must be in coordinate order."""
    import sys
    from .. import aln, parallel
    quantize = _check_qmap(quantize)
    if bam_index is not None:
        check_bam_index_options(bam_index, bam_out, output)
    if bam_out:
        if _bgzf.enabled():
            raise ValueError('--bam-out: not with --bgzf (a BAM file is a BGZF file already)')
        if parallel.launched_from_env() or parallel.world_rank()[0] > 1:
            raise ValueError(BAM_OUT_RANKS)
    elif output is not None and str(output).lower().endswith('.bam'):
        raise ValueError('applybqsr writes SAM text; BAM output (%s) is not supported' % output)
    if not isinstance(bam, aln.AlignmentFile):
        # (with bam_out and KBBQ_GPU_BAM=1 a BAM file's records are decoded on the device and stay there as records for the
        # writer: kbbq/_bamin.py; in every other case this IS AlignmentFile(bam))
        bam = aln.alignments(bam, device=None if bam_out else False, planes=('seq', 'oq') if use_oq else ('seq', 'qual', 'oq'),
                             keep_stream=True)
    if bam_out:
        *model, rg_to_int = report_model(bam, report_path)
        kw = dict(use_oq=use_oq, set_oq=set_oq)
        if quantize is not None:
            kw['quantize'] = quantize
        if isinstance(bam, aln.DeviceAlignments):
            kw['resident'] = device_resident(bam, use_oq)
        write_bam_file(bam, output, lambda writer: write_alignments_bam(bam, *model, rg_to_int, writer, **kw),
                       **({} if bam_index is None else {'index': bam_index}))
        return
    world, rank = parallel.world_rank()
    if world > 1 and output is None:
        raise ValueError('several ranks need -o: every rank writes OUTPUT.rankNNNN')
    *model, rg_to_int = report_model(bam, report_path)
    lo, hi = parallel.shard_range(len(bam), rank, world) if world > 1 else (0, len(bam))
    kw = dict(use_oq=use_oq, set_oq=set_oq, rows=(lo, hi), header=rank == 0)
    if quantize is not None:                                 # without it the call is the one it was
        kw['quantize'] = quantize
    if output is None and _bgzf.enabled():
        with _bgzf.stdout_sink() as sink:
            write_alignments(bam, *model, rg_to_int, sink, **kw)
        return
    if output is None:
        sys.stdout.flush()
        write_alignments(bam, *model, rg_to_int, sys.stdout.buffer, **kw)
        sys.stdout.flush()
        return
    with _bgzf.open_sink(output if world == 1 else '%s.rank%04d' % (output, rank)) as sink:
        write_alignments(bam, *model, rg_to_int, sink, **kw)
