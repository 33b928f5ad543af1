"""CPU model of `kbbq bqsr --kmers` (kbbq.gatk.bqsr.bam_to_kmer_covariates): the loop of oracle_bqsr.bam_to_bqsr_covariates with
the errors taken from kmer_model.correct over the SEQ plane of ALL records (soft clips included) instead of a reference, and
the skips true outside the aligned part.  A test helper only: the product has no CPU fallback."""
import numpy as np

import kmer_model as M

from test_oracle_bqsr import VEC                      # noqa: E402,F401  (the nine vectors' names)
FIXTURE = dict(seed=11, npairs=300, S=60, contigs=(('chr1', 800), ('chr2', 700)))      # 600 records, about 24x coverage


def load(sam):
    """(reads, read-group IDs in header order, PU names in header order) of a SAM file, through the oracle's stand-ins."""
    import _shim
    bam = _shim.AlignmentFile(sam)
    rgs = bam.as_dict()['RG']
    return list(bam), [rg['ID'] for rg in rgs], [rg['PU'] for rg in rgs]


def planes(reads):
    """(SEQ plane, meta words) of all records."""
    return M.plane([r.query_sequence.encode('ascii') for r in reads])


def flags(reads, k, t=None):
    """(error plane bool [n, pitch], t): where kmer_model.correct changes a base of the SEQ plane."""
    seq, meta = planes(reads)
    out, _, t = M.correct(seq, meta, k, t)
    return out != seq, t


def vectors(reads, rg_ids, k, t=None, use_oq=False, minscore=6, maxscore=42, no_errors=False, flagged=None):
    """(the nine vectors, info): info = dict(min_count, flagged_bases over all bases, bases).  no_errors: all flags forced to 0.
    flagged: what flags(reads, k, t) returned, for callers that keep it."""
    import oracle as O
    import oracle_bqsr as OQ
    err, t = flagged if flagged is not None else flags(reads, k, t)
    flagged = err
    if no_errors:
        err = np.zeros_like(err)
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
            if i < a or i >= b or q[i] < minscore or trimmed[i] or read.query_sequence[i] == 'N':
                continue
            expected[rg] += O.q_to_p(np.array([q[i]]))[0]
            e = bool(err[r, i])
            rg_t[rg] += 1; q_t[rg, q[i]] += 1; p_t[rg, q[i], pos[i]] += 1
            if e:
                rg_e[rg] += 1; q_e[rg, q[i]] += 1; p_e[rg, q[i], pos[i]] += 1
            if dn[i] != -1:
                d_t[rg, q[i], dn[i]] += 1
                if e:
                    d_e[rg, q[i], dn[i]] += 1
    with np.errstate(all='ignore'):
        meanq = O.p_to_q(expected / rg_t)
    info = dict(min_count=t, flagged_bases=int(flagged.sum()), bases=len(reads) * S)
    return (meanq, rg_e, rg_t, q_e, q_t, p_e, p_t, d_e, d_t), info


def check_share(info):
    """A degenerate fixture must fail, not pass vacuously: the model flags 1 %..10 % of all bases."""
    share = info['flagged_bases'] / info['bases']
    assert 0.01 <= share <= 0.10, (info, share)
    return share
