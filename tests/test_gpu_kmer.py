"""kbbq correct on the MI355X: the device k-mer table, histogram, threshold and corrected plane against the CPU model
(tests/kmer_model.py), the full-table error, the host-buffer slab path and the command line feeding `recalibrate -f`."""
import os
import sys

import numpy as np
import pytest

import kmer_model as M

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
def test_table_histogram_and_threshold_equal_the_model(reads, k):
    from kbbq import kmer
    seq, meta = reads[:2]
    keys, counts = M.count(seq, meta, k)
    table = kmer.count_kmers(_device(seq), _device(meta), k=k)
    gk, gc = table.entries()
    assert np.array_equal(gk, keys) and np.array_equal(gc.astype(np.int64), counts)
    h = kmer.kmer_histogram(table)
    assert np.array_equal(h, M.histogram(counts))
    assert kmer.solid_threshold(h) == M.threshold(M.histogram(counts))
    table.close()


@pytest.mark.parametrize('k', [21, 31])
def test_corrected_plane_equals_the_model(reads, k):
    from kbbq import kmer
    seq, meta = reads[:2]
    want, want_changed, t = M.correct(seq, meta, k)
    out, info = kmer.correct_reads(_device(seq), _device(meta), k=k)
    assert info['min_count'] == t
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(info['changed'].cpu().numpy().astype(np.int64), want_changed)
    host, hinfo = kmer.correct_reads(seq, meta, k=k)
    assert np.array_equal(host, want) and np.array_equal(hinfo['changed'].astype(np.int64), want_changed)


def test_recall_and_precision(reads):
    from kbbq import kmer
    seq, meta, truth, errs = reads
    out, info = kmer.correct_reads(seq, meta, k=31)
    touched = out != seq
    recall = (errs & (out == truth)).sum() / errs.sum()
    precision = (touched & (out == truth)).sum() / max(touched.sum(), 1)
    assert recall >= 0.85 and precision >= 0.99, (recall, precision)
    assert int(info['changed'].sum()) == int(touched.sum())


def test_too_few_slots_raise_and_return(reads):
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = reads[:2]
    for plane, m in ((seq, meta), (_device(seq), _device(meta))):
        with pytest.raises(N.KmerTableFull, match='slots'):
            kmer.count_kmers(plane, m, k=31, slots=1024)
    # the context is usable afterwards
    keys, counts = M.count(seq[:50], meta[:50], 21)
    gk, gc = kmer.count_kmers(seq[:50], meta[:50], k=21).entries()
    assert np.array_equal(gk, keys) and np.array_equal(gc.astype(np.int64), counts)


def test_table_that_does_not_fit_names_slots(reads, monkeypatch):
    from kbbq import kmer
    monkeypatch.setenv('KBBQ_DEVICE_BUDGET', '1M')
    with pytest.raises(ValueError, match='slots'):
        kmer.count_kmers(reads[0], reads[1], k=31, slots=1 << 20)


def test_many_slabs_equal_one(reads, monkeypatch):
    from kbbq import kmer
    seq, meta = reads[:2]
    one_t = kmer.count_kmers(seq, meta, k=31)
    one = one_t.entries()
    one_out, one_info = kmer.correct_reads(seq, meta, k=31)
    monkeypatch.setenv('KBBQ_STAGE_MB', '1')               # slabs of a few thousand rows
    many = kmer.count_kmers(seq, meta, k=31).entries()
    assert np.array_equal(many[0], one[0]) and np.array_equal(many[1], one[1])
    out, info = kmer.correct_reads(seq, meta, k=31)
    assert np.array_equal(out, one_out) and np.array_equal(info['changed'], one_info['changed'])
    # counting adds: two halves into one table equal the whole
    t2 = kmer.KmerTable(31, one_t.slots)
    h = seq.shape[0] // 2
    kmer.count_kmers(seq[:h], meta[:h], table=t2)
    kmer.count_kmers(seq[h:], meta[h:], table=t2)
    two = t2.entries()
    assert np.array_equal(two[0], one[0]) and np.array_equal(two[1], one[1])


def _kbbq(*argv, timeout=600):
    import subprocess
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=env)


def test_cli_correct_then_recalibrate(reads, tmp_path):
    import gzip
    order = np.argsort(reads[1], kind='stable')          # recalibrate -f takes reads of non-decreasing length (the reference's rule)
    seq, meta = reads[0][order], reads[1][order]
    n = seq.shape[0]
    rng = np.random.default_rng(3)
    qual = (rng.integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    names = ['r%d' % i for i in range(n)]
    lens = meta.astype(np.int64)

    def text(plane):
        return ''.join('@%s\n%s\n+\n%s\n' % (names[i], plane[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                       for i in range(n))

    fq = tmp_path / 'reads.fq'
    fq.write_text(text(seq))
    want, _, t = M.correct(seq, meta, 31)
    r = _kbbq('correct', '-f', str(fq))
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == text(want)
    assert ('min_count=%d' % t) in r.stderr.decode()
    gz = tmp_path / 'reads.fq.gz'
    gz.write_bytes(gzip.compress(fq.read_bytes()))
    cor = tmp_path / 'reads.cor.fq'
    r = _kbbq('correct', '-f', str(gz), '-k', '31', '-o', str(cor))
    assert r.returncode == 0, r.stderr.decode()
    assert cor.read_text() == text(want)
    r = _kbbq('recalibrate', '-f', str(fq), str(cor))
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().count('\n+\n') == n
    env_world = dict(WORLD_SIZE='2')
    import subprocess
    r2 = subprocess.run([sys.executable, '-m', 'kbbq.main', 'correct', '-f', str(fq)], capture_output=True, timeout=120,
                        env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'), **env_world))
    assert r2.returncode != 0 and b'one GPU' in r2.stderr
