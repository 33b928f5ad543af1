"""kbbq correct across ranks on the MI355X.  One process: tables of three shards routed by select(nbuckets=3) into three
owner tables with merge equal the CPU model (tests/kmer_model.py), and so do the summed histograms, the solid select and the
corrected plane against the gathered solid table.  Ranks (gloo, three ranks sharing the GPU, as tests/test_gpu_ranks.py):
`kbbq correct` writes the bytes and the summary line of one process -- to rank files and to stdout, from .fq.gz, with
--min-count, in several counting rounds -- and so does a one-rank RCCL group; a table too small stops every rank; the rank
files feed `recalibrate -f` on three ranks as the one-process file does."""
import glob
import gzip
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = 3


@pytest.fixture(scope='module')
def reads():
    return M.synth(7, genome_len=20000, depth=30, err=0.01, len_lo=36, len_hi=300)


def _routed(seq, meta, k, world=3):
    """Owner tables of `world` shards counted apart and routed by owner."""
    from kbbq import _device as dev
    from kbbq import kmer
    slots = kmer.default_slots(kmer.kmer_total(meta, k), dev.device_budget())
    owners = [kmer.KmerTable(k, slots) for _ in range(world)]
    for rows in np.array_split(np.arange(seq.shape[0]), world):
        local = kmer.count_kmers(seq[rows], meta[rows], k=k)
        keys, counts, sizes = kmer.select(local, nbuckets=world)
        assert int(sizes.sum()) == local.entries()[0].size
        lo = 0
        for j in range(world):
            hi = lo + int(sizes[j])
            kmer.merge(owners[j], keys[lo:hi], counts[lo:hi])
            lo = hi
        local.close()
    return owners


@pytest.mark.parametrize('k', [21, 31])
def test_routed_owner_tables_equal_the_model(reads, k):
    from kbbq import kmer
    seq, meta = reads[:2]
    want_keys, want_counts = M.count(seq, meta, k)
    owners = _routed(seq, meta, k)
    parts = [t.entries() for t in owners]
    for j, (keys, _) in enumerate(parts):
        assert keys.size and np.all(kmer.owner(keys, 3) == j)
    keys = np.concatenate([p[0] for p in parts])
    counts = np.concatenate([p[1] for p in parts]).astype(np.int64)
    order = np.argsort(keys)
    assert np.array_equal(keys[order], want_keys) and np.array_equal(counts[order], want_counts)
    hist = sum(kmer.kmer_histogram(t) for t in owners)
    assert np.array_equal(hist, M.histogram(want_counts))
    t = kmer.solid_threshold(hist)
    assert t == M.threshold(M.histogram(want_counts))
    # the solid select of every owner table, gathered into one table: the model's solid set, and the model's correction
    sel = [kmer.select(o, nbuckets=1, min_count=t) for o in owners]
    sk = np.concatenate([s[0].cpu().numpy().view(np.uint64) for s in sel])
    sc = np.concatenate([s[1].cpu().numpy() for s in sel]).astype(np.int64)
    assert sum(int(s[2][0]) for s in sel) == sk.size
    order = np.argsort(sk)
    solid = want_counts >= t
    assert np.array_equal(sk[order], want_keys[solid]) and np.array_equal(sc[order], want_counts[solid])
    table = kmer.KmerTable(k, kmer.default_slots(sk.size, 1 << 40))
    for s in sel:
        kmer.merge(table, s[0], s[1])
    for o in owners:
        o.close()
    out, changed = kmer.correct_with(table, seq, meta, t)
    want, want_changed, wt = M.correct(seq, meta, k)
    assert wt == t
    assert np.array_equal(out, want) and np.array_equal(changed.astype(np.int64), want_changed)
    table.close()


def test_select_buckets_are_dense_and_in_owner_order(reads):
    from kbbq import kmer
    seq, meta = reads[:2]
    table = kmer.count_kmers(seq, meta, k=25)
    keys, counts, sizes = kmer.select(table, nbuckets=1000, min_count=2)
    k = keys.cpu().numpy().view(np.uint64)
    own = kmer.owner(k, 1000)
    assert np.array_equal(own, np.repeat(np.arange(1000, dtype=np.uint32), sizes))
    wk, wc = table.entries()
    assert np.array_equal(np.sort(k), wk[wc >= 2])
    with pytest.raises(ValueError, match='nbuckets'):
        kmer.select(table, nbuckets=1025)
    table.close()


def test_merge_into_a_small_table_raises_and_clear_empties(reads):
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = reads[:2]
    table = kmer.count_kmers(seq, meta, k=31)
    keys, counts, _ = kmer.select(table)
    with pytest.raises(N.KmerTableFull, match='give more slots'):
        kmer.merge(kmer.KmerTable(31, 1024), keys, counts)
    table.clear()
    assert table.entries()[0].size == 0
    # the context and the cleared table count as new
    kmer.count_kmers(seq[:100], meta[:100], table=table)
    gk, gc = table.entries()
    wk, wc = M.count(seq[:100], meta[:100], 31)
    assert np.array_equal(gk, wk) and np.array_equal(gc.astype(np.int64), wc)
    table.close()


# ---- ranks ------------------------------------------------------------------------------------------------------------------

def _port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _launch(world, script, argv, env=None, timeout=400):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'), **(env or {}))
    env.setdefault('KBBQ_DIST_BACKEND', 'gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr',
           '127.0.0.1', '--master-port', str(_port()), os.path.join(ROOT, 'tests', script)] + list(argv)
    return subprocess.run(cmd, env=env, capture_output=True, timeout=timeout)


def _ranks(argv, **kw):
    return _launch(RANKS, 'dist_cli_worker.py', argv, **kw)


def _one(*argv, timeout=400):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS')}
    env['PYTHONPATH'] = os.path.join(ROOT, 'kbbq-py_amd')
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=env)


def _summary(stderr):
    return re.findall(r'^kbbq correct: k=.*$', stderr.decode(), flags=re.M)


@pytest.fixture(scope='module')
def fastq(reads, tmp_path_factory):
    """reads.fq (shortest reads first: `recalibrate -f` takes non-decreasing lengths), its .gz and the one-process output."""
    d = tmp_path_factory.mktemp('kmer_ranks')
    order = np.argsort(reads[1], kind='stable')
    seq, meta = reads[0][order], reads[1][order]
    n = seq.shape[0]
    qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    lens = meta.astype(np.int64)
    fq = d / 'reads.fq'
    fq.write_text(''.join('@r%d\n%s\n+\n%s\n' % (i, seq[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                          for i in range(n)))
    gz = d / 'reads.fq.gz'
    gz.write_bytes(gzip.compress(fq.read_bytes()))
    ref = d / 'one.fq'
    r = _one('correct', '-f', str(fq), '-o', str(ref))
    assert r.returncode == 0, r.stderr.decode()
    r3 = _one('correct', '-f', str(fq), '--min-count', '3', '-o', str(d / 'one_m3.fq'))
    assert r3.returncode == 0, r3.stderr.decode()
    return dict(dir=d, fq=str(fq), gz=str(gz), ref=ref.read_bytes(), line=_summary(r.stderr), seq=seq, meta=meta,
                ref_m3=(d / 'one_m3.fq').read_bytes(), line_m3=_summary(r3.stderr))


def _joined(out, world=RANKS):
    parts = sorted(glob.glob(out + '.rank*'))
    assert len(parts) == world, parts
    return b''.join(open(p, 'rb').read() for p in parts)


@pytest.mark.parametrize('case', ['file', 'stdout', 'gz', 'min_count', 'rounds'])
def test_ranks_write_the_one_process_bytes(fastq, case, tmp_path):
    from kbbq import kmer
    src = fastq['gz'] if case == 'gz' else fastq['fq']
    argv = ['correct', '-f', src]
    want, line = fastq['ref'], fastq['line']
    if case == 'min_count':
        argv += ['--min-count', '3']
        want, line = fastq['ref_m3'], fastq['line_m3']
    if case == 'rounds':
        local = 1 << 15                  # 16 Ki windows a round: every rank's share (about a third of all) takes 3 or more
        assert kmer.kmer_total(fastq['meta'], 31) / RANKS * 0.8 >= 3 * local * kmer.LOAD_FACTOR
        argv += ['--local-slots', str(local)]
    out = str(tmp_path / 'out.fq')
    if case != 'stdout':
        argv += ['-o', out]
    r = _ranks(argv)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = r.stdout if case == 'stdout' else _joined(out)
    if case != 'stdout':
        assert r.stdout == b''
    assert got == want
    assert len(line) == 1 and _summary(r.stderr) == line


def test_owner_tables_of_the_ranks_equal_the_model(fastq, tmp_path):
    """count_kmers_ranks on three ranks, in rounds: every rank holds exactly the model's counts of the keys it owns; the summed
    histogram is the model's."""
    from kbbq import kmer
    out = str(tmp_path / 'owned')
    r = _launch(RANKS, 'dist_kmer_worker.py', [fastq['fq'], '27', str(1 << 14), out])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    want_keys, want_counts = M.count(fastq['seq'], fastq['meta'], 27)
    parts = [np.load('%s.rank%04d.npz' % (out, j)) for j in range(RANKS)]
    for j, p in enumerate(parts):
        assert p['keys'].size and np.all(kmer.owner(p['keys'], RANKS) == j)
        assert np.array_equal(p['hist'], M.histogram(want_counts))
    assert sum(int(p['reads']) for p in parts) == fastq['seq'].shape[0]
    keys = np.concatenate([p['keys'] for p in parts])
    counts = np.concatenate([p['counts'] for p in parts]).astype(np.int64)
    order = np.argsort(keys)
    assert np.array_equal(keys[order], want_keys) and np.array_equal(counts[order], want_counts)


def test_one_rank_over_rccl(fastq, tmp_path):
    """A group of ONE rank over RCCL (KBBQ_DIST_ALWAYS=1, backend nccl): the exchange, the gathers and the sums with device
    tensors through librccl; the rank writes -o itself, as `recalibrate` does."""
    out = str(tmp_path / 'out.fq')
    r = _launch(1, 'dist_cli_worker.py', ['correct', '-f', fastq['fq'], '-o', out],
                env=dict(KBBQ_DIST_ALWAYS='1', KBBQ_DIST_BACKEND='nccl'), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert open(out, 'rb').read() == fastq['ref']
    assert _summary(r.stderr) == fastq['line']


def test_a_full_table_stops_every_rank(fastq, tmp_path):
    r = _ranks(['correct', '-f', fastq['fq'], '--slots', '1024', '-o', str(tmp_path / 'out.fq')], timeout=300)
    err = r.stderr.decode()
    assert r.returncode != 0
    for j in range(RANKS):
        assert re.search(r'kbbq correct: rank %d: .*give more slots' % j, err), err[-3000:]


def test_rank_files_feed_recalibrate_on_ranks(fastq, tmp_path):
    one = _one('recalibrate', '-f', fastq['fq'], str(fastq['dir'] / 'one.fq'))
    assert one.returncode == 0, one.stderr.decode()
    out = str(tmp_path / 'cor.fq')
    r = _ranks(['correct', '-f', fastq['fq'], '-o', out])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    cor = tmp_path / 'cor_all.fq'
    cor.write_bytes(_joined(out))
    rec = str(tmp_path / 'rec.fq')
    r = _ranks(['recalibrate', '-f', fastq['fq'], str(cor), '-o', rec])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert _joined(rec) == one.stdout
