"""The k-mer prefilter's host side, no GPU: the hash (kbbq.kmer.filter_index) against the independent model, the filter's
sizing, the model's own guarantee (no k-mer seen twice is lost), the command line's new flags and the refusals that must come
before any device call."""
import numpy as np
import pytest

import kmer_model as M
import kmer_prefilter_model as P


@pytest.fixture(scope='module')
def reads():
    return M.synth(7, genome_len=20000, depth=30, err=0.01, len_lo=36, len_hi=300)


def test_filter_index_equals_the_model():
    from kbbq import kmer
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 62, size=5000, dtype=np.uint64)
    keys[:4] = [0, 1, (1 << 62) - 1, 0xFFFFFFFFFFFFFFFE]
    for words in (1, 2, 1 << 10, 1 << 20, 1 << 33):
        w, m = kmer.filter_index(keys, words)
        mw, mm = P.filter_index(keys, words)
        assert w.dtype == np.uint64 and m.dtype == np.uint64
        assert np.array_equal(w.astype(np.int64), mw) and np.array_equal(m, mm)
        assert int(w.max()) < words
        for i in range(0, 5000, 499):                    # ... and both against plain Python integers
            assert (int(w[i]), int(m[i])) == P.index_one(keys[i], words)
    bits = np.array([bin(int(x)).count('1') for x in m])
    assert bits.min() >= 1 and bits.max() <= 4 and (bits == 4).mean() > 0.8
    # a salt of its own: neither the home slot's hash nor the owner's
    assert kmer.FILTER_SALT == P.SALT and kmer.FILTER_SALT != kmer.OWNER_SALT
    with pytest.raises(ValueError, match='words'):
        kmer.filter_index(keys, 3)


def test_filter_words():
    from kbbq import kmer
    assert kmer.filter_words(0) == 1 and kmer.filter_words(16) == 1 and kmer.filter_words(17) == 2
    assert kmer.filter_words(478609) == 32768                                # 4 bits: 1,914,436 bits -> 2^15 words
    assert kmer.filter_words(478609, 8) == 65536 and kmer.filter_words(478609, 1) == 8192
    assert kmer.filter_words(16_000_000 * 120) == 1 << 27                    # 1 byte per window: 2 x 1 GiB
    for total, bits in ((1, 1), (1000, 4), (12345, 7), (1 << 20, 64)):
        w = kmer.filter_words(total, bits)
        assert w == P.filter_words(total, bits) and w & (w - 1) == 0 and w * 64 >= bits * total and (w == 1 or w * 32 < bits * total)
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match='filter_bits'):
            kmer.filter_words(100, bad)


@pytest.mark.parametrize('k', [15, 31])
def test_simulation_admits_every_key_seen_twice(reads, k):
    seq, meta = reads[:2]
    keys, counts = M.count(seq, meta, k)
    words = P.filter_words(int(counts.sum()))
    rng = np.random.default_rng(2)
    for order in (None, rng.permutation(seq.shape[0])):
        seen, twice, admitted = P.simulate(P.stream(seq, meta, k, order), words)
        assert np.array_equal(seen, P.seen_expected(keys, words))
        assert not np.any(twice & ~seen)
        got = P.in_filter(keys, twice)
        assert got[counts >= 2].all()
        single = int((counts == 1).sum())
        assert int(got[counts == 1].sum()) <= 0.05 * single
        assert admitted <= int(got.sum())                # an OR into `twice` sets a new bit once per key at most


def test_argparse_takes_the_new_flags(monkeypatch):
    from kbbq import kmer, main
    calls = []
    monkeypatch.setattr(kmer, 'main_correct', lambda *a, **kw: calls.append((a, kw)))
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the command then leaves the memory back end alone
    main.main(['correct', '-f', 'x.fq'])
    main.main(['correct', '-f', 'x.fq', '--prefilter'])
    main.main(['correct', '-f', 'x.fq', '--prefilter', '--filter-bits', '8', '--min-count', '3'])
    assert [(kw['prefilter'], kw['filter_bits'], kw['min_count']) for _, kw in calls] == [(False, 4, None), (True, 4, None), (True, 8, 3)]


def _no_device(monkeypatch):
    from kbbq import _native, kmer

    def boom(*a, **kw):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(kmer, '_ctx', boom)
    monkeypatch.setattr(_native, 'load', boom)
    monkeypatch.setattr(kmer, 'prefilter_kmers', boom)
    monkeypatch.setattr(kmer, 'count_kmers', boom)


def test_min_count_one_is_refused_before_any_device_call(reads, monkeypatch, tmp_path):
    from kbbq import kmer
    _no_device(monkeypatch)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    seq, meta = reads[:2]
    for mc in (1, 0):
        with pytest.raises(ValueError, match='min_count'):
            kmer.correct_reads(seq, meta, k=31, min_count=mc, prefilter=True)
        with pytest.raises(ValueError, match='min_count'):
            kmer.correct_fastq(str(tmp_path / 'absent.fq'), str(tmp_path / 'out.fq'), min_count=mc, prefilter=True)
        with pytest.raises(ValueError, match='min_count'):
            kmer.main_correct(str(tmp_path / 'absent.fq'), min_count=mc, prefilter=True)
    with pytest.raises(ValueError, match='filter_bits'):
        kmer.correct_reads(seq, meta, k=31, prefilter=True, filter_bits=0)


def test_ranks_refuse_the_prefilter_before_any_collective(reads, monkeypatch, tmp_path):
    from kbbq import kmer, parallel
    _no_device(monkeypatch)

    def collective(*a, **kw):
        raise AssertionError('a collective was started')
    for name in ('all_gather_object', 'sum_over_ranks', 'max_over_ranks', 'raise_first_error', 'barrier', 'all_to_all_rows'):
        monkeypatch.setattr(parallel, name, collective)
    monkeypatch.setattr(kmer, '_read_shard', collective)
    seq, meta = reads[:2]
    for rank in (0, 1):                                  # every rank refuses, not rank 0 alone
        monkeypatch.setattr(kmer, '_ranks', lambda rank=rank: (2, rank))
        with pytest.raises(ValueError, match='ranks'):
            kmer.correct_reads(seq, meta, k=31, prefilter=True)
        with pytest.raises(ValueError, match='ranks'):
            kmer.correct_fastq(str(tmp_path / 'absent.fq'), str(tmp_path / 'out.fq'), prefilter=True)
        with pytest.raises(ValueError, match='owns the key'):
            kmer.main_correct(str(tmp_path / 'absent.fq'), min_count=3, prefilter=True)
