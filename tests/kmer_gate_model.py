"""CPU model of the quality gate (`--kmer-min-qual Q`; include/kbbq_hip.h kbbq_kmer_gate_rows_dev), built on kmer_model: a base
is countable when it is A/C/G/T and its quality byte is >= byte_min (Q + 33 for character qualities), a window is counted iff
all k of its bases are countable.  gate() writes 'N' where the quality byte is below byte_min -- every other byte as read -- and
the counts, the histogram and the threshold are kmer_model's of that plane; the correction is kmer_model.correct of the plane AS
READ with the solid set taken from the gated count.  A test helper only.  Also the two fixtures the tests share."""
import numpy as np

import kmer_model as M


def gate(seq, qual, byte_min):
    """The gated plane: `seq` with 'N' wherever qual < byte_min (padding included: its quality byte is 0)."""
    out = np.array(seq, dtype=np.uint8, copy=True)
    out[np.asarray(qual, dtype=np.uint8) < byte_min] = ord('N')
    return out


def count(seq, qual, meta, k, byte_min):
    """(keys uint64 sorted, counts int64) of the counted windows."""
    return M.count(gate(seq, qual, byte_min), meta, k)


def counted_windows(seq, qual, meta, k, byte_min):
    """The number of counted windows: the sum of count()'s counts."""
    return int(M.windows(gate(seq, qual, byte_min), meta, k)[2].sum())


class _PlainIndices:
    """NumPy with nonzero() handing out Python ints: kmer_model.correct shifts by up to 2 (k - 1) bits with an index taken from
    np.nonzero, which overflows an int64 at k = 32 where the Python int the model means does not."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def nonzero(x):
        return tuple(a.tolist() for a in np.nonzero(x))


def correct(seq, qual, meta, k, byte_min, t=None):
    """(corrected plane, per-read changed counts, t): kmer_model.correct of the rows as read against the gated count -- the
    threshold is the gated histogram's first valley unless given, and every window of the rows as read is looked up."""
    gated = count(seq, qual, meta, k, byte_min)
    plain, M.count, M.np = M.count, (lambda s, m, kk: gated), _PlainIndices()
    try:
        return M.correct(seq, meta, k, t)
    finally:
        M.count, M.np = plain, np


def quals(seq, meta):
    """The fixtures' quality plane: {2, 12, 23, 37} + 33 with shares .5 / 1 / 3.5 / 95 %, byte 0 at and beyond each length."""
    q = (np.random.default_rng(5).choice([2, 12, 23, 37], size=seq.shape, p=[.005, .01, .035, .95]) + 33).astype(np.uint8)
    lens = np.asarray(meta, dtype=np.uint32).astype(np.int64) & 0xFFFF
    q[np.arange(seq.shape[1])[None, :] >= lens[:, None]] = 0
    return q


# name -> (synth's len_lo, len_hi, Q, k)
FIXTURES = {'F1': (150, 150, 24, 21), 'F2': (36, 300, 20, 31)}
_memo = {}


def fixture(name):
    """A fixture and everything the model says about it, computed once and left unchanged: a dict of seq, qual, meta, Q, k,
    gated (plane), keys / counts / hist / t (of the gated count), windows (counted), plain_keys / plain_t / plain_windows and
    plain_out (the run without the option), out / changed (the gated correction)."""
    if name not in _memo:
        lo, hi, Q, k = FIXTURES[name]
        seq, meta = M.synth(11, genome_len=5000, depth=30, err=0.01, len_lo=lo, len_hi=hi)[:2]
        qual = quals(seq, meta)
        keys, counts = count(seq, qual, meta, k, Q + 33)
        hist = M.histogram(counts)
        out, changed, t = correct(seq, qual, meta, k, Q + 33)
        pk, pc = M.count(seq, meta, k)
        M.np = _PlainIndices()
        try:
            pout, _, pt = M.correct(seq, meta, k)
        finally:
            M.np = np
        f = dict(seq=seq, qual=qual, meta=meta, Q=Q, k=k, gated=gate(seq, qual, Q + 33), keys=keys, counts=counts, hist=hist, t=t,
                 windows=counted_windows(seq, qual, meta, k, Q + 33), plain_keys=pk, plain_t=pt, plain_windows=int(pc.sum()),
                 plain_out=pout, out=out, changed=changed)
        for v in f.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _memo[name] = f
    return _memo[name]


def assert_not_vacuous(f):
    """What every test asserts of its case: some but not all bases are gated, the gated table has fewer keys than the ungated
    one, and the correction changes at least one base."""
    lens = f['meta'].astype(np.int64) & 0xFFFF
    inside = np.arange(f['seq'].shape[1])[None, :] < lens[:, None]
    low = inside & (f['qual'] < f['Q'] + 33)
    assert 0 < int(low.sum()) < int(inside.sum())
    assert 0 < f['keys'].size < f['plain_keys'].size
    assert int(f['changed'].sum()) > 0


# ---------------------------------------------------------------- aligned records (bqsr --kmers, recalibrate -b --kmers, benchmark --kmers)
def aligned_quals(reads, pitch, use_oq=False, exclude=None):
    """The quality plane (characters, byte 0 behind every record) of the records that are not excluded: QUAL, or the OQ tag."""
    import oracle_bqsr as OQ
    keep = [i for i in range(len(reads)) if exclude is None or not exclude[i]]
    qual = np.zeros((len(keep), pitch), dtype=np.uint8)
    for row, i in enumerate(keep):
        q = OQ.read_oq(reads[i]) if use_oq else np.array(reads[i].query_qualities, dtype=np.int64)
        qual[row, :len(q)] = q + 33
    return qual


def solid(seq, qual, meta, k, byte_min, t=None):
    """(sorted solid keys, t) of the gated count: t is its histogram's first valley unless given."""
    keys, counts = count(seq, qual, meta, k, byte_min)
    if t is None:
        t = M.threshold(M.histogram(counts))
    return keys[counts >= t], t


def classify(seq, qual, meta, k, byte_min, t=None, passes=1):
    """(class plane, t) of the rows AS READ against the gated count (kmer_unresolved_model.classify; passes > 1:
    kmer_passes_model.passes): 0 trusted / break, 1 the correction ends on another letter, 2 unresolved."""
    keys, t = solid(seq, qual, meta, k, byte_min, t)
    if passes > 1:
        import kmer_passes_model as PM
        return PM.passes(seq, meta, k, t, passes, solid_keys=keys)[2], t
    import kmer_unresolved_model as U
    return U.classify(seq, meta, k, t, solid_keys=keys)[0], t


def aligned_classes(reads, k, Q, t=None, use_oq=False, exclude=None):
    """kmer_mixed_model.flags with the gate in front of the count and the unresolved bases told apart: (class plane uint8
    [n, pitch] over ALL records -- rows of excluded ones all 0 --, t, counted windows).  The k-mers are counted from the gated
    SEQ plane of the records that are not excluded (their QUAL, or OQ tag, decides); SEQ as read is judged."""
    import kmer_mixed_model as MX
    seq, meta, keep = MX.planes(reads, exclude)
    qual = aligned_quals(reads, seq.shape[1], use_oq, exclude)
    part, t = classify(seq, qual, meta, k, Q + 33, t)
    cls = np.zeros((len(reads), seq.shape[1]), dtype=np.uint8)
    cls[keep] = part
    return cls, t, counted_windows(seq, qual, meta, k, Q + 33)
