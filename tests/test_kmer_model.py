"""The CPU model of kbbq correct (tests/kmer_model.py) on hand-made cases: the GPU tests compare against it byte for byte."""
import numpy as np
import pytest

import kmer_model as M


def _genome(seed, n):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, n)])


def _tiled(g, L, step):
    return [g[s:s + L] for s in range(0, len(g) - L + 1, step)]


def _with(read, i, b):
    return read[:i] + bytes([b]) + read[i + 1:]


def _other(b):
    return M.LETTERS[(M.LETTERS.index(b) + 1) % 4]


def test_single_error_at_10x_is_fixed():
    k = 15
    g = _genome(1, 400)
    reads = [g[60:160]] * 10
    bad = _with(g[60:160], 50, _other(g[110]))
    seq, meta = M.plane(reads + [bad])
    out, changed, t = M.correct(seq, meta, k, t=2)
    assert bytes(out[-1, :100]) == g[60:160]
    assert changed.tolist() == [0] * 10 + [1]
    assert np.array_equal(out[:10], seq[:10])


def test_a_tie_leaves_the_base_unchanged():
    k = 9
    g = _genome(2, 60)
    a, c = _with(g, 30, ord('A') if g[30] != ord('A') else ord('C')), None
    alt = [b for b in M.LETTERS if b not in (g[30], a[30])]
    c = _with(g, 30, alt[0])
    # two alternatives equally solid, the read itself holds the third letter
    seq, meta = M.plane([a] * 5 + [c] * 5 + [_with(g, 30, alt[1])])
    out, changed, _ = M.correct(seq, meta, k, t=2)
    assert out[-1, 30] == alt[1] and changed[-1] == 0


@pytest.mark.parametrize('read', [b'ACGTACGTAC', b'N' * 40, b'acgtacgtacgtacgtacgtacgtacgt'])
def test_short_n_and_lowercase_reads_are_unchanged(read):
    k = 15
    g = _genome(3, 200)
    seq, meta = M.plane([g] * 5 + [read])
    out, changed, _ = M.correct(seq, meta, k, t=2)
    assert np.array_equal(out, seq) and changed.sum() == 0
    _, _, valid = M.windows(seq[-1:], meta[-1:], k)
    assert not valid.any()


def test_two_errors_five_apart_are_both_fixed():
    k = 11
    g = _genome(4, 300)
    reads = _tiled(g, 100, 4) * 3
    bad = g[100:200]
    bad = _with(_with(bad, 40, _other(bad[40])), 45, _other(bad[45]))
    seq, meta = M.plane(reads + [bad])
    out, changed, _ = M.correct(seq, meta, k, t=2)
    assert bytes(out[-1, :100]) == g[100:200] and changed[-1] == 2


def test_k32_palindrome_is_counted_once_per_occurrence():
    half = b'ACGTTGCAAGGCTTAC'
    pal = half + bytes(M.LETTERS[3 - M.LETTERS.index(b)] for b in reversed(half))   # its own reverse complement
    fwd = 0
    for b in pal:
        fwd = fwd << 2 | M.LETTERS.index(b)
    assert M.revcomp(fwd, 32) == fwd
    seq, meta = M.plane([pal, pal, pal])
    keys, counts = M.count(seq, meta, 32)
    assert keys.tolist() == [fwd] and counts.tolist() == [3]


def test_counts_are_canonical():
    seq, meta = M.plane([b'AAAAAAAAAC', b'GTTTTTTTTT'])        # reverse complements of each other
    keys, counts = M.count(seq, meta, 10)
    assert keys.tolist() == [1] and counts.tolist() == [2]


def test_valley_rule():
    h = np.zeros(257, dtype=np.int64)
    h[1:8] = [1000, 300, 50, 60, 70, 40, 10]
    assert M.threshold(h) == 3
    h = np.zeros(257, dtype=np.int64)
    h[1:5] = [100, 20, 20, 5]
    assert M.threshold(h) == 2                                  # equal counts are a valley
    h = np.zeros(257, dtype=np.int64)
    h[1:] = np.arange(256, 0, -1)                               # strictly falling: no valley
    with pytest.raises(ValueError):
        M.threshold(h)


def test_model_recovers_most_errors():
    seq, meta, truth, errs = M.synth(5, genome_len=8000, depth=30)
    out, changed, t = M.correct(seq, meta, 31)
    fixed = errs & (out == truth)
    touched = out != seq
    assert fixed.sum() / errs.sum() >= 0.85
    assert (touched & (out == truth)).sum() / max(touched.sum(), 1) >= 0.99
    assert changed.sum() == touched.sum()
