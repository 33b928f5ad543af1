"""CPU model of the three outcomes of the k-mer rule for a base (include/kbbq_hip.h, kbbq_kmer_flag_ex_dev with
KBBQ_KMER_FLAG_UNRESOLVED), written from the contract on top of kmer_model's windows and counts: NumPy over the windows that
cover every untrusted base, one pass per (offset in the window, substitution).  0 trusted / break / padding, 1 error (one
substitution makes strictly the most covering k-mers solid, >= 1), 2 unresolved (untrusted, and no substitution wins).  Also
the nine vectors of `kbbq bqsr --kmers --skip-unresolved`: kmer_bqsr_model.vectors' loop with the class-2 bases left out of
errors and totals.  A test helper only: the product has no CPU fallback."""
import numpy as np

import kmer_model as M


def _revcomp(fwd, k):
    """Reverse-complement codes of an array of forward codes (first base in the high bits)."""
    f = np.asarray(fwd, dtype=np.uint64)
    r = np.zeros_like(f)
    for i in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - ((f >> np.uint64(2 * i)) & np.uint64(3)))
    return r


def classify(seq, meta, k, t=None, solid_keys=None):
    """(class plane uint8 [n, pitch], per-read count of 1s, per-read count of 2s, t).  solid_keys: judge the rows against this
    sorted set of solid canonical keys instead of their own counts (t is then returned as given)."""
    seq = np.asarray(seq, dtype=np.uint8)
    if solid_keys is None:
        keys, counts = M.count(seq, meta, k)
        if t is None:
            t = M.threshold(M.histogram(counts))
        solid_keys = keys[counts >= t]
    solid_keys = np.asarray(solid_keys, dtype=np.uint64)

    def is_solid(canon):
        if not solid_keys.size:
            return np.zeros(np.shape(canon), dtype=bool)
        i = np.minimum(np.searchsorted(solid_keys, canon), solid_keys.size - 1)
        return solid_keys[i] == canon

    fwd, canon, valid = M.windows(seq, meta, k)
    c = M._codes(seq, meta)
    n, pitch = seq.shape
    W = fwd.shape[1]
    cls = np.zeros((n, pitch), dtype=np.uint8)
    ones = np.zeros(n, dtype=np.int64)
    twos = np.zeros(n, dtype=np.int64)
    if W == 0 or n == 0:
        return cls, ones, twos, t
    solid = valid & is_solid(canon)
    # base i is covered by the windows starting in [i - k + 1, i] that exist
    cs_s = np.zeros((n, W + 1), dtype=np.int64)
    cs_v = np.zeros((n, W + 1), dtype=np.int64)
    np.cumsum(solid, axis=1, out=cs_s[:, 1:])
    np.cumsum(valid, axis=1, out=cs_v[:, 1:])
    p = np.arange(pitch)
    lo = np.maximum(p - k + 1, 0)
    hi = np.maximum(np.minimum(p, W - 1) + 1, lo)
    untrusted = (c < 4) & ((cs_v[:, hi] - cs_v[:, lo]) > 0) & ((cs_s[:, hi] - cs_s[:, lo]) == 0)
    rr, ii = np.nonzero(untrusted)
    if rr.size == 0:
        return cls, ones, twos, t
    rc = _revcomp(fwd, k)
    score = np.zeros((rr.size, 4), dtype=np.int64)       # [:, x]: solid covering windows with the base's code XOR x written
    for d in range(k):                                   # the base is the d-th base of the window starting at i - d
        j = ii - d
        ok = (j >= 0) & (j < W)
        jj = np.clip(j, 0, W - 1)
        ok &= valid[rr, jj]
        f, r = fwd[rr, jj], rc[rr, jj]
        for x in (1, 2, 3):
            ff = f ^ (np.uint64(x) << np.uint64(2 * (k - 1 - d)))
            rx = r ^ (np.uint64(x) << np.uint64(2 * d))  # the complement of a base changes by the same XOR
            score[:, x] += ok & is_solid(np.minimum(ff, rx))
    top = score[:, 1:].max(axis=1)
    winner = (top >= 1) & ((score[:, 1:] == top[:, None]).sum(axis=1) == 1)
    cls[rr, ii] = np.where(winner, 1, 2)
    ones = (cls == 1).sum(axis=1).astype(np.int64)
    twos = (cls == 2).sum(axis=1).astype(np.int64)
    return cls, ones, twos, t


def classes(reads, k, t=None):
    """(class plane, t) of the SEQ plane of all records of a file (kmer_bqsr_model.planes)."""
    import kmer_bqsr_model as B
    seq, meta = B.planes(reads)
    cls, _, _, t = classify(seq, meta, k, t)
    return cls, t


def vectors(reads, rg_ids, k, t=None, use_oq=False, minscore=6, maxscore=42, classified=None):
    """(the nine vectors, info) of bam_to_kmer_covariates(skip_unresolved=True): the loop of kmer_bqsr_model.vectors with the
    class-1 bases as errors and the class-2 bases in neither errors nor totals.  info = dict(min_count, flagged_bases,
    skipped_bases -- both over all bases of SEQ --, bases).  classified: what classes(reads, k, t) returned."""
    import oracle as O
    import oracle_bqsr as OQ
    cls, t = classified if classified is not None else classes(reads, k, t)
    rg_to_int = {rg: i for i, rg in enumerate(rg_ids)}
    R = len(rg_ids)
    S = len(reads[0].query_sequence)
    expected = np.zeros(R, dtype=np.longdouble)
    rg_e = np.zeros(R, dtype=np.int64); rg_t = np.zeros(R, dtype=np.int64)
    q_e = np.zeros((R, maxscore + 1), dtype=np.int64); q_t = np.zeros_like(q_e)
    p_e = np.zeros((R, maxscore + 1, 2 * S), dtype=np.int64); p_t = np.zeros_like(p_e)
    d_e = np.zeros((R, maxscore + 1, 16), dtype=np.int64); d_t = np.zeros_like(d_e)
    for r, read in enumerate(reads):
        rg = rg_to_int[read.get_tag('RG')]
        q = OQ.read_oq(read) if use_oq else np.array(read.query_qualities, dtype=np.int64)
        pos = OQ.bqsr_cycle(read)
        dn = OQ.bqsr_dinuc(read, use_oq=use_oq)
        trimmed = OQ.trim(read)
        assert len(q) == S and read.query_length == S
        a, b = read.query_alignment_start, read.query_alignment_end
        for i in range(S):
            if i < a or i >= b or q[i] < minscore or trimmed[i] or read.query_sequence[i] == 'N' or cls[r, i] == 2:
                continue
            expected[rg] += O.q_to_p(np.array([q[i]]))[0]
            e = cls[r, i] == 1
            rg_t[rg] += 1; q_t[rg, q[i]] += 1; p_t[rg, q[i], pos[i]] += 1
            if e:
                rg_e[rg] += 1; q_e[rg, q[i]] += 1; p_e[rg, q[i], pos[i]] += 1
            if dn[i] != -1:
                d_t[rg, q[i], dn[i]] += 1
                if e:
                    d_e[rg, q[i], dn[i]] += 1
    with np.errstate(all='ignore'):
        meanq = O.p_to_q(expected / rg_t)
    info = dict(min_count=t, flagged_bases=int((cls == 1).sum()), skipped_bases=int((cls == 2).sum()), bases=len(reads) * S)
    return (meanq, rg_e, rg_t, q_e, q_t, p_e, p_t, d_e, d_t), info
