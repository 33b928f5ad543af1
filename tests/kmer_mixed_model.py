"""CPU model of `kbbq bqsr --kmers --mixed-lengths [-F INT]` (kbbq.gatk.bqsr.bam_to_kmer_covariates with mixed_lengths / exclude_flags):
kmer_bqsr_model.vectors without its one-length assertion.  S is the longest SEQ of the file, every record is walked over its own
length, and a negative cycle -(c + 1) wraps into the axis of 2 S as NumPy wraps it: column 2 S - 1 - c, whatever the record's
length.  Records under the `exclude` mask are left out of the plane the k-mers are counted and judged on, and out of the loop; they
still count into S.  On a file of one length with no exclusions the result is kmer_bqsr_model.vectors' own.  A test helper only: the
product has no CPU fallback.

flagged=(plane, t) is kmer_bqsr_model's parameter; here the plane may also be a class plane of tests/kmer_passes_model.py (1 an error,
2 unresolved): the class-2 bases are then left out of the tally the way tests/kmer_skip_model.py states it, by a quality below
minscore at the base itself."""
import numpy as np

import kmer_model as M
import kmer_skip_model as K

from kmer_bqsr_model import VEC, FIXTURE, load, check_share           # noqa: F401  (what the tests of both models share)


def planes(reads, exclude=None):
    """(SEQ plane of the records that are not excluded, meta words, their indices)."""
    keep = [i for i in range(len(reads)) if exclude is None or not exclude[i]]
    longest = max(len(r.query_sequence) for r in reads)
    seq, meta = M.plane([reads[i].query_sequence.encode('ascii') for i in keep], pitch=max(16, (longest + 15) // 16 * 16))
    return seq, meta, np.array(keep, dtype=np.int64)


def flags(reads, k, t=None, exclude=None):
    """(error plane bool [n, pitch] over ALL records -- rows of excluded ones all False --, t)."""
    seq, meta, keep = planes(reads, exclude)
    out, _, t = M.correct(seq, meta, k, t)
    err = np.zeros((len(reads), seq.shape[1]), dtype=bool)
    err[keep] = out != seq
    return err, t


def vectors(reads, rg_ids, k, t=None, use_oq=False, minscore=6, maxscore=42, exclude=None, flagged=None):
    """(the nine vectors, info): info = dict(min_count, flagged_bases and skipped_bases over all bases of the records that are not
    excluded, bases, excluded_reads)."""
    import oracle as O
    import oracle_bqsr as OQ
    exclude = np.zeros(len(reads), dtype=bool) if exclude is None else np.asarray(exclude, dtype=bool)
    plane, t = flagged if flagged is not None else flags(reads, k, t, exclude)
    plane = np.asarray(plane).astype(np.uint8)
    assert plane.shape[0] == len(reads) and not plane[exclude].any()
    rg_to_int = {rg: i for i, rg in enumerate(rg_ids)}
    R = len(rg_ids)
    S = max(len(r.query_sequence) for r in reads)
    expected = np.zeros(R, dtype=np.longdouble)
    rg_e = np.zeros(R, dtype=np.int64); rg_t = np.zeros(R, dtype=np.int64)
    q_e = np.zeros((R, maxscore + 1), dtype=np.int64); q_t = np.zeros_like(q_e)
    p_e = np.zeros((R, maxscore + 1, 2 * S), dtype=np.int64); p_t = np.zeros_like(p_e)
    d_e = np.zeros((R, maxscore + 1, 16), dtype=np.int64); d_t = np.zeros_like(d_e)
    bases = 0
    for r, read in enumerate(reads):
        if exclude[r]:
            continue
        rg = rg_to_int[read.get_tag('RG')]
        L = len(read.query_sequence)
        q = OQ.read_oq(read) if use_oq else np.array(read.query_qualities, dtype=np.int64)
        assert len(q) == L and read.query_length == L and 1 <= L <= S
        assert not plane[r, L:].any()
        bases += L
        # an unresolved base is skipped like a base below minscore (kmer_skip_model): its neighbours keep their contexts
        q = K.masked_quals((q + 33).astype(np.uint8), plane[r, :L]).astype(np.int64) - 33
        pos = OQ.bqsr_cycle(read)
        dn = OQ.bqsr_dinuc(read, use_oq=use_oq)
        trimmed = OQ.trim(read)
        a, b = read.query_alignment_start, read.query_alignment_end
        assert 0 <= a and b <= L
        for i in range(L):
            if i < a or i >= b or q[i] < minscore or trimmed[i] or read.query_sequence[i] == 'N':
                continue
            assert -S <= pos[i] < S
            expected[rg] += O.q_to_p(np.array([q[i]]))[0]
            e = plane[r, i] == 1
            rg_t[rg] += 1; q_t[rg, q[i]] += 1; p_t[rg, q[i], pos[i]] += 1          # a negative cycle wraps into 2 S
            if e:
                rg_e[rg] += 1; q_e[rg, q[i]] += 1; p_e[rg, q[i], pos[i]] += 1
            if dn[i] != -1:
                d_t[rg, q[i], dn[i]] += 1
                if e:
                    d_e[rg, q[i], dn[i]] += 1
    with np.errstate(all='ignore'):
        meanq = O.p_to_q(expected / rg_t)
    info = dict(min_count=t, flagged_bases=int((plane == 1).sum()), skipped_bases=int((plane == 2).sum()), bases=bases,
                excluded_reads=int(exclude.sum()))
    return (meanq, rg_e, rg_t, q_e, q_t, p_e, p_t, d_e, d_t), info


# ---------------------------------------------------------------- fixtures: records shortened the way a trimmer leaves them
_QUERY, _REF = 'MIS=X', 'MDN=X'


def _ops(cigar):
    out, num = [], ''
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append([int(num), ch]); num = ''
    return out


def cut(fields, length, at_start):
    """The SAM fields of a record with SEQ, QUAL, the OQ tag and the CIGAR cut to `length` query bases -- from the end of the stored
    SEQ, or from its start (POS then advances by the reference bases removed).  No H operation is added; an operation that
    consumes no query base is not left at the cut end."""
    f = list(fields)
    L = len(f[9])
    drop = L - length
    assert 0 < length <= L
    if drop == 0:
        return f
    ops = _ops(f[5])
    assert sum(n for n, o in ops if o in _QUERY) == L
    if at_start:
        ops.reverse()
    gone_ref = 0
    while drop > 0 or ops[-1][1] not in _QUERY:
        n, o = ops[-1]
        if o not in _QUERY:                                   # a deletion at the cut end goes with the bases behind it
            gone_ref += n; ops.pop()
            continue
        take = min(n, drop)
        drop -= take
        gone_ref += take if o in _REF else 0
        if take == n:
            ops.pop()
        else:
            ops[-1][0] = n - take
    if at_start:
        ops.reverse()
        f[3] = str(int(f[3]) + gone_ref)
    f[5] = ''.join('%d%s' % (n, o) for n, o in ops)
    sl = slice(L - length, None) if at_start else slice(0, length)
    f[9], f[10] = f[9][sl], f[10][sl]
    for j in range(11, len(f)):
        if f[j].startswith('OQ:Z:'):
            f[j] = 'OQ:Z:' + f[j][5:][sl]
    assert sum(n for n, o in ops if o in _QUERY) == length == len(f[9]) == len(f[10])
    return f


MIXED_LENGTHS = (60, 59, 48, 47, 33, 32, 31, 17, 16, 14)
SHORT_LENGTHS = (31, 30, 24, 17, 16)


def shorten(sam_text, which):
    """The SAM text with records cut: 'mixed' -- every third record to a length cycling through MIXED_LENGTHS, the cuts alternating
    between the stored SEQ's end and its start; 'short' -- every record, lengths cycling through SHORT_LENGTHS, alternating too."""
    out, idx, ncut = [], 0, 0
    for ln in sam_text.split('\n'):
        if ln and not ln.startswith('@'):
            if which == 'short' or idx % 3 == 0:
                lengths = SHORT_LENGTHS if which == 'short' else MIXED_LENGTHS
                ln = '\t'.join(cut(ln.split('\t'), lengths[ncut % len(lengths)], at_start=bool((ncut // len(lengths) + ncut) % 2)))
                ncut += 1
            idx += 1
        out.append(ln)
    return '\n'.join(out)
