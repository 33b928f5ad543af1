"""kbbq correct --prefilter on the MI355X: the filter's arrays against the CPU model (tests/kmer_prefilter_model.py), the
filtered table, histogram, threshold and corrected plane against the unfiltered model (tests/kmer_model.py), the smaller
table, and the command line.

Measured by the builder on one MI355X, k = 31 on the fixture below: see DESIGN.md, "Prefilter"."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M
import kmer_prefilter_model as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def reads():
    return M.synth(7, genome_len=20000, depth=30, err=0.01, len_lo=36, len_hi=300)


def _device(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


@pytest.mark.parametrize('k', [15, 21, 31, 32])
def test_filter_arrays_against_the_model(reads, k):
    from kbbq import kmer
    seq, meta = reads[:2]
    keys, counts = M.count(seq, meta, k)
    f = kmer.prefilter_kmers(_device(seq), _device(meta), k=k)
    by_length = int(np.maximum(meta.astype(np.int64) - k + 1, 0).sum())     # the windows by length, those an N breaks included
    assert f.words == P.filter_words(by_length) and f.nbytes == 16 * f.words
    seen, twice = f.download()
    admitted = f.admitted
    assert np.array_equal(seen, P.seen_expected(keys, f.words))
    assert P.in_filter(keys[counts >= 2], twice).all()
    assert not np.any(twice & ~seen)
    print('k=%d words=%d admitted=%d keys in twice=%d (count >= 2: %d, singletons: %d)'
          % (k, f.words, admitted, int(P.in_filter(keys, twice).sum()), int((counts >= 2).sum()), int((counts == 1).sum())))
    # the host-buffer path fills the same `seen`; clear() empties the filter
    f.clear()
    assert not f.download()[0].any() and not f.download()[1].any() and f.admitted == 0
    kmer.prefilter_kmers(seq, meta, k=k, filter=f)
    hseen, htwice = f.download()
    assert np.array_equal(hseen, seen) and P.in_filter(keys[counts >= 2], htwice).all() and not np.any(htwice & ~hseen)
    f.release_seen()
    assert f.download()[0] is None and f.nbytes == 8 * f.words
    f.close()


@pytest.mark.parametrize('k', [15, 21, 31, 32])
def test_filtered_table_histogram_and_threshold(reads, k):
    from kbbq import kmer
    seq, meta = reads[:2]
    keys, counts = M.count(seq, meta, k)
    dseq, dmeta = _device(seq), _device(meta)
    f = kmer.prefilter_kmers(dseq, dmeta, k=k)
    table = kmer.count_kmers(dseq, dmeta, k=k, filter=f)
    gk, gc = table.entries()
    gc = gc.astype(np.int64)
    assert np.array_equal(gk[gc >= 2], keys[counts >= 2]) and np.array_equal(gc[gc >= 2], counts[counts >= 2])
    singles = keys[counts == 1]
    got1 = gk[gc == 1]
    print('k=%d slots=%d entries=%d of them count 1: %d of %d singletons (%.3f %%)'
          % (k, table.slots, gk.size, got1.size, singles.size, 100.0 * got1.size / singles.size))
    assert np.isin(got1, singles).all()
    assert got1.size <= 0.05 * singles.size
    assert not (gc < 1).any()
    h = kmer.kmer_histogram(table)
    want = M.histogram(counts)
    assert np.array_equal(h[2:], want[2:]) and h[1] == got1.size and h[0] == 0
    assert kmer.solid_threshold(h) == M.threshold(want)
    table.close()
    f.close()


@pytest.mark.parametrize('k', [21, 31])
def test_corrected_plane_equals_the_model(reads, k, monkeypatch):
    from kbbq import kmer
    seq, meta = reads[:2]
    want, want_changed, t = M.correct(seq, meta, k)
    out, info = kmer.correct_reads(_device(seq), _device(meta), k=k, prefilter=True)
    assert info['min_count'] == t and info['prefilter'] is True and info['admitted'] > 0
    assert info['filter_bytes'] == 16 * P.filter_words(kmer.kmer_total(meta, k))
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(info['changed'].cpu().numpy().astype(np.int64), want_changed)
    host, hinfo = kmer.correct_reads(seq, meta, k=k, prefilter=True)
    assert np.array_equal(host, want) and np.array_equal(hinfo['changed'].astype(np.int64), want_changed)
    monkeypatch.setenv('KBBQ_STAGE_MB', '1')               # slabs of a few thousand rows, each of the three passes
    many, minfo = kmer.correct_reads(seq, meta, k=k, prefilter=True)
    assert np.array_equal(many, want) and np.array_equal(minfo['changed'].astype(np.int64), want_changed)
    assert minfo['min_count'] == t and np.array_equal(minfo['hist'][2:], hinfo['hist'][2:])
    # without the prefilter the info says so
    _, plain = kmer.correct_reads(seq, meta, k=k)
    assert plain['prefilter'] is False and plain['filter_bytes'] == 0 and plain['admitted'] is None
    assert np.array_equal(plain['hist'][2:], hinfo['hist'][2:])


def test_default_table_is_a_quarter_or_less(reads):
    from kbbq import kmer
    seq, meta = reads[:2]
    _, plain = kmer.correct_reads(seq, meta, k=31)
    _, filt = kmer.correct_reads(seq, meta, k=31, prefilter=True)
    print('slots without %d, with %d; admitted %d' % (plain['slots'], filt['slots'], filt['admitted']))
    assert filt['slots'] * 4 <= plain['slots']
    assert filt['table_bytes'] * 4 <= plain['table_bytes']


def test_a_table_too_small_for_the_plain_count_serves_the_filtered_one(reads):
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = reads[:2]
    with pytest.raises(N.KmerTableFull, match='slots'):
        kmer.count_kmers(seq, meta, k=31, slots=1 << 16)
    want, want_changed, t = M.correct(seq, meta, 31)
    out, info = kmer.correct_reads(seq, meta, k=31, slots=1 << 16, prefilter=True)
    assert info['slots'] == 1 << 16 and info['min_count'] == t
    assert np.array_equal(out, want) and np.array_equal(info['changed'].astype(np.int64), want_changed)


def test_a_filtered_table_that_fills_still_says_so(reads):
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = reads[:2]
    with pytest.raises(N.KmerTableFull, match='slots'):
        kmer.correct_reads(seq, meta, k=31, slots=1 << 12, prefilter=True)      # 22,594 keys of count >= 2 alone do not fit
    out, info = kmer.correct_reads(seq[:50], meta[:50], k=21, min_count=2, prefilter=True)   # the context is usable afterwards
    assert np.array_equal(out, M.correct(seq[:50], meta[:50], 21, 2)[0])


def _kbbq(*argv, timeout=600):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=env)


def test_cli_prefilter_writes_the_same_bytes(reads, tmp_path):
    from kbbq import kmer
    order = np.argsort(reads[1], kind='stable')          # recalibrate -f takes reads of non-decreasing length
    seq, meta = reads[0][order], reads[1][order]
    n = seq.shape[0]
    rng = np.random.default_rng(3)
    qual = (rng.integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    lens = meta.astype(np.int64)
    fq = tmp_path / 'reads.fq'
    fq.write_text(''.join('@r%d\n%s\n+\n%s\n' % (i, seq[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                          for i in range(n)))
    plain = _kbbq('correct', '-f', str(fq))
    assert plain.returncode == 0, plain.stderr.decode()
    assert b'prefilter' not in plain.stderr
    r = _kbbq('correct', '-f', str(fq), '--prefilter')
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == plain.stdout and len(r.stdout) > 0
    line = [x for x in r.stderr.decode().splitlines() if x.startswith('kbbq correct:')][-1]
    pline = [x for x in plain.stderr.decode().splitlines() if x.startswith('kbbq correct:')][-1]
    assert line.startswith(pline + ' prefilter=1 admitted=') and ' slots=' in line
    cor = tmp_path / 'reads.cor.fq'
    r = _kbbq('correct', '-f', str(fq), '--prefilter', '--filter-bits', '8', '-o', str(cor))
    assert r.returncode == 0, r.stderr.decode()
    assert cor.read_bytes() == plain.stdout
    r = _kbbq('recalibrate', '-f', str(fq), str(cor))
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().count('\n+\n') == n
    r = _kbbq('correct', '-f', str(fq), '--min-count', '1', '--prefilter')
    assert r.returncode != 0 and b'min_count' in r.stderr and r.stdout == b''
    # in-process: a refused call leaves the context usable
    with pytest.raises(ValueError, match='min_count'):
        kmer.correct_reads(seq, meta, k=31, min_count=1, prefilter=True)
    out, _ = kmer.correct_reads(seq[:50], meta[:50], k=21, min_count=2, prefilter=True)
    assert np.array_equal(out, M.correct(seq[:50], meta[:50], 21, 2)[0])


def test_larger_set_equals_the_plain_path():
    from kbbq import kmer
    seq, meta = M.synth(11, genome_len=200000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
    dseq, dmeta = _device(seq), _device(meta)
    plain_out, plain = kmer.correct_reads(dseq, dmeta, k=31)
    out, info = kmer.correct_reads(dseq, dmeta, k=31, prefilter=True)
    print('reads %d: threshold %d; slots without %d, with %d; admitted %d; h[1] without %d, with %d'
          % (seq.shape[0], info['min_count'], plain['slots'], info['slots'], info['admitted'], plain['hist'][1], info['hist'][1]))
    assert info['min_count'] == plain['min_count']
    assert np.array_equal(info['hist'][2:], plain['hist'][2:])
    assert np.array_equal(info['changed'].cpu().numpy(), plain['changed'].cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), plain_out.cpu().numpy())
    assert info['hist'][1] <= 0.05 * plain['hist'][1]
    assert info['slots'] * 4 <= plain['slots']
