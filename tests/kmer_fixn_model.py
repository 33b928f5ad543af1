"""CPU model of the N rule of kbbq correct --fix-n (include/kbbq_hip.h, KBBQ_KMER_FIX_N), written from the contract: plain NumPy
and Python integers on top of kmer_model.windows / kmer_model.count for keys and counts.  A test helper only: the product has
no CPU fallback.  Also the N-carrying read set the GPU tests use (with_ns) with its hand-placed cases.

The rule.  Counting and the threshold know nothing of it.  An 'N' at base i of a read has the candidate windows [s, s + k) with
s <= i < s + k that lie inside the read and hold no other base outside A/C/G/T; for each letter x the number of candidate
windows whose canonical k-mer with x written at i has a count >= t is taken, and the N becomes the letter with the strictly
largest number when that is >= 1.  Everything is judged against the read as read; a fixed N is a changed base."""
import numpy as np

import kmer_model as M

NCH = ord('N')
KINDS = ('fixed', 'tie', 'none', 'second_break', 'no_window')


class _PlainIndices:
    """NumPy as kmer_model sees it, with nonzero() handing out Python ints: M.correct shifts by 2 (k - 1 - (i - j)) with i taken
    from np.nonzero, and at k = 32 a NumPy int64 shifted by 62 overflows where the Python int the model means does not."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def nonzero(x):
        return tuple(a.tolist() for a in np.nonzero(x))


_RC4 = [sum((3 - ((b >> (2 * j)) & 3)) << (2 * (3 - j)) for j in range(4)) for b in range(256)]


def revcomp(f, k):
    """kmer_model.revcomp of a Python integer, four bases at a step."""
    y = 0
    for b in range(8):
        y |= _RC4[(f >> (8 * b)) & 255] << (8 * (7 - b))
    return y >> (64 - 2 * k)


def substitutions(seq, meta, k, t=None):
    """kmer_model.correct (the substitution rule alone), safe at k = 32 and with the quick revcomp (the same function)."""
    slow = M.revcomp
    M.np, M.revcomp = _PlainIndices(), revcomp
    try:
        return M.correct(seq, meta, k, t)
    finally:
        M.np, M.revcomp = np, slow


def correct(seq, meta, k, t=None, fix_n=True, sep=None):
    """(corrected plane, per-row changed counts, t, kinds): kmer_model.correct plus, with fix_n, the N rule.  sep: per row, the
    index of a base that is a separator and no N (a row of two reads), or None.  kinds: {(row, base): one of KINDS} of every N
    inside a read, {} without fix_n."""
    seq = np.asarray(seq, dtype=np.uint8)
    out, changed, t = substitutions(seq, meta, k, t)
    kinds = {}
    if not fix_n:
        return out, changed, t, kinds
    keys, counts = M.count(seq, meta, k)
    solid = set(keys[counts >= t].tolist())
    fwd, _, _ = M.windows(seq, meta, k)                  # a break's code is 0 in the forward word
    c = M._codes(seq, meta)
    lens = (np.asarray(meta, dtype=np.uint32).astype(np.int64) & 0xFFFF).tolist()
    rows, cols = np.nonzero((seq == NCH) & (np.arange(seq.shape[1])[None, :] < np.asarray(lens)[:, None]))
    for r, i in zip(rows.tolist(), cols.tolist()):
        if sep is not None and sep[r] is not None and int(sep[r]) == i:
            continue
        L = lens[r]
        inside = [s for s in range(max(0, i - k + 1), min(i, L - k) + 1)]
        cand = [s for s in inside if int((c[r, s:s + k] == 4).sum()) == 1]
        if not cand:
            kinds[(r, i)] = 'second_break' if inside else 'no_window'
            continue
        score = []
        for x in range(4):
            tot = 0
            for s in cand:
                f = int(fwd[r, s]) | (x << (2 * (k - 1 - (i - s))))
                tot += min(f, revcomp(f, k)) in solid
            score.append(tot)
        best = max(score)
        if best >= 1 and score.count(best) == 1:
            out[r, i] = M.LETTERS[score.index(best)]
            changed[r] += 1
            kinds[(r, i)] = 'fixed'
        else:
            kinds[(r, i)] = 'tie' if best >= 1 else 'none'
    return out, changed, t, kinds


def kind_counts(kinds):
    return {name: sum(1 for v in kinds.values() if v == name) for name in KINDS}


def _letters(x):
    return np.frombuffer(M.LETTERS, dtype=np.uint8)[x]


def with_ns(seed, k, genome_len=20000, depth=30, n_rate=0.002, copies=24):
    """kmer_model.synth reads (errors and its own few Ns) with more bases overwritten by N at random, plus hand-placed cases
    written over rows of their own: (seq plane, meta, cases) with cases = {name: (row, base)}.

    Placed on error-free rows of at least 2 k + 48 bases: an N at base 0, at the last base and at bases 15, 16, 31 and 32 (the
    16-byte chunk edges); two Ns d apart for d in 1, k - 1, k, k + 1.  A row cut to exactly k bases and one cut to k - 1, each
    with an N.  'tie': two variants of a fresh 2 k + 1-base segment that differ in the middle base, `copies` reads of each, and
    one more read of it with an N there: the letters tie.  'errors': an N whose neighbours on both sides are substitution errors,
    so every candidate window holds one and no letter makes a solid k-mer."""
    seq, meta, truth, _ = M.synth(seed, genome_len=genome_len, depth=depth, err=0.01, len_lo=36, len_hi=300)
    rng = np.random.default_rng(seed + 1000)
    seq, meta = seq.copy(), meta.copy()
    lens = meta.astype(np.int64)
    pitch = seq.shape[1]
    inside = np.arange(pitch)[None, :] < lens[:, None]
    seq[inside & (rng.random(seq.shape) < n_rate)] = NCH
    cases = {}
    long_rows = iter(np.nonzero(lens >= 2 * k + 48)[0].tolist())

    def clean():
        r = next(long_rows)
        seq[r] = truth[r]
        return r, int(lens[r])
    for name, at in (('first', 0), ('last', -1), ('b15', 15), ('b16', 16), ('b31', 31), ('b32', 32)):
        r, L = clean()
        i = at % L
        seq[r, i] = NCH
        cases[name] = (r, i)
    for d in (1, k - 1, k, k + 1):
        r, L = clean()
        seq[r, 37] = seq[r, 37 + d] = NCH
        cases['pair_d%d' % d] = (r, 37)
        cases['pair_d%d_second' % d] = (r, 37 + d)
    for name, L in (('exactly_k', k), ('shorter_than_k', k - 1)):
        r, _ = clean()
        seq[r, L:] = NCH
        meta[r] = L
        lens[r] = L
        seq[r, L // 2] = NCH
        cases[name] = (r, L // 2)
    r, L = clean()
    i = L // 2
    for j in (i - 1, i + 1):
        seq[r, j] = _letters((M._CODE[truth[r, j]] + 1) % 4)
    seq[r, i] = NCH
    cases['errors'] = (r, i)
    # two variants at equal depth, and a read with an N at the site
    W = 2 * k + 1
    seg = rng.integers(0, 4, W).astype(np.uint8)
    rows = np.full((2 * copies + 1, pitch), NCH, dtype=np.uint8)
    for v in range(2):
        x = seg.copy()
        x[k] = (seg[k] + v) % 4
        rows[v * copies:(v + 1) * copies, :W] = _letters(x)
    rows[-1, :W] = _letters(seg)
    rows[-1, k] = NCH
    cases['tie'] = (seq.shape[0] + 2 * copies, k)
    seq = np.concatenate([seq, rows])
    meta = np.concatenate([meta, np.full(2 * copies + 1, W, dtype=np.uint32)])
    return seq, meta, cases
