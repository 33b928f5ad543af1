"""CPU model of `kbbq benchmark --kmers` (kbbq.benchmark.benchmark_kmers): the joint array joint[q][truth error][k-mer class]
from oracle_benchmark.find_read_errors per record (truth error, truth skip), kmer_unresolved_model.classes over the SEQ plane
of ALL records (class plane and threshold) and the record's qualities; also the text table and the stderr line, written from
their definitions.  A test helper only: the product has no CPU fallback."""
import numpy as np

COLUMNS = ('#predicted_q', 'bases', 'errors', 'flagged', 'flagged_errors', 'unresolved', 'unresolved_errors', 'actual_q', 'kmer_q',
           'kmer_q_skip', 'label')


def load(paths, bed=False):
    """(reads, ref, skips) of a truth set's files through the oracle's stand-in readers; bed: everything outside conf.bed is skipped."""
    import _shim
    import oracle_benchmark as OB
    reads = list(_shim.AlignmentFile(paths['sam']))
    ref = OB.get_ref_dict(paths['fa'])
    skips = OB.get_full_skips(ref, OB.get_var_sites(paths['vcf']), paths['bed'] if bed else None)
    return reads, ref, skips


def qualities(read, use_oq):
    if use_oq:
        return np.array([ord(c) - 33 for c in read.get_tag('OQ')], dtype=np.int64)
    return np.array(read.query_qualities, dtype=np.int64)


def joint(reads, ref, skips, k, t=None, use_oq=False, classified=None):
    """(joint int64 [256, 2, 3], info).  classified: what kmer_unresolved_model.classes(reads, k, t) returned, for callers that
    keep it (it depends on neither the qualities nor the skips).  info: k, min_count, reads and the six totals."""
    import kmer_unresolved_model as U
    import oracle_benchmark as OB
    cls, t = classified if classified is not None else U.classes(reads, k, t)
    J = np.zeros((256, 2, 3), dtype=np.int64)
    for r, read in enumerate(reads):
        err, skip = OB.find_read_errors(read, ref, skips)
        q = qualities(read, use_oq)
        n = len(read.query_sequence)
        assert len(q) == n == len(err)
        keep = ~skip
        np.add.at(J, (q[keep], err[keep].astype(np.int64), cls[r, :n][keep].astype(np.int64)), 1)
    return J, dict(k=k, min_count=int(t), reads=len(reads), **totals(J))


def totals(J):
    S = J.sum(axis=0)
    return dict(bases=int(S.sum()), errors=int(S[1].sum()), flagged=int(S[:, 1].sum()), flagged_errors=int(S[1, 1]),
                unresolved=int(S[:, 2].sum()), unresolved_errors=int(S[1, 2]))


def _q(a, b):
    import oracle as O
    return int(O.p_to_q(np.array([a / b]))[0])


def render(J, label):
    """The table `kbbq benchmark --kmers` prints, as one string."""
    out = ['\t'.join(COLUMNS)]
    for q in range(256):
        C = J[q]
        bases = int(C.sum())
        if bases == 0:
            continue
        errors, flagged, unresolved = int(C[1].sum()), int(C[:, 1].sum()), int(C[:, 2].sum())
        skipq = _q(flagged, bases - unresolved) if bases - unresolved else 0
        out.append('\t'.join(str(x) for x in (q, bases, errors, flagged, int(C[1, 1]), unresolved, int(C[1, 2]), _q(errors, bases),
                                              _q(flagged, bases), skipq, label)))
    return '\n'.join(out) + '\n'


def summary(info, prefilter=None):
    """The stderr line.  prefilter: (admitted, slots) for the suffix of --prefilter."""
    ratio = lambda a, b: a / b if b else 0.0
    line = 'kbbq benchmark: k=%d min_count=%d reads=%d' % (info['k'], info['min_count'], info['reads'])
    for name in ('bases', 'errors', 'flagged', 'flagged_errors', 'unresolved', 'unresolved_errors'):
        line += ' %s=%d' % (name, info[name])
    line += ' precision=%.4f recall=%.4f' % (ratio(info['flagged_errors'], info['flagged']), ratio(info['flagged_errors'], info['errors']))
    if prefilter is not None:
        line += ' prefilter=1 admitted=%d slots=%d' % prefilter
    return line
