"""`kbbq correct --kmers-from SET` across ranks on the MI355X (gloo, two ranks sharing the GPU, launched as
tests/test_gpu_kmer_ranks.py launches its own): the rank files concatenated are the one-process bytes, for a set counted plainly and
for one counted on one GPU with --prefilter --partitions 2, which ranks cannot count themselves; a corrupt set makes every rank
exit non-zero, each naming the pair, and nobody hangs."""
import glob
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M
import kmer_set_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = 2
K = 15


def _port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _ranks(argv, timeout=240):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
    env.setdefault('KBBQ_DIST_BACKEND', 'gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(RANKS), '--master-addr',
           '127.0.0.1', '--master-port', str(_port()), os.path.join(ROOT, 'tests', 'dist_kmer_set_worker.py')] + list(argv)
    return subprocess.run(cmd, env=env, capture_output=True, timeout=timeout)


def _one(*argv, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS')}
    env['PYTHONPATH'] = os.path.join(ROOT, 'kbbq-py_amd')
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=env)


def _summary(stderr):
    return re.findall(r'^kbbq correct: k=.*$', stderr.decode(), flags=re.M)


@pytest.fixture(scope='module')
def fastq(tmp_path_factory):
    """reads.fq, two sets of it (one counted plainly, one with --prefilter --partitions 2) and the one-process output."""
    d = tmp_path_factory.mktemp('kmer_set_ranks')
    seq, meta = M.synth(29, genome_len=2000, depth=30, err=0.01, len_lo=40, len_hi=70)[:2]
    lens = meta.astype(np.int64)
    records = [(seq[i, :lens[i]].tobytes(), b'I' * int(lens[i])) for i in range(seq.shape[0])]
    fq = d / 'reads.fq'
    fq.write_bytes(b''.join(b'@r%d\n%s\n+\n%s\n' % (i, s, q) for i, (s, q) in enumerate(records)))
    want_set = SM.set_bytes(records, K, 2)
    f = SM.parse(want_set)
    assert M.threshold(f['hist']) >= 2                               # the valley the runs below rely on
    plain, parts = d / 'plain.set', d / 'parts.set'
    for path, more in ((plain, ()), (parts, ('--prefilter', '--partitions', '2'))):
        r = _one('count', '-f', str(fq), '-k', str(K), '-o', str(path), *more)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert path.read_bytes() == want_set
    ref = d / 'one.fq'
    r = _one('correct', '-f', str(fq), '-k', str(K), '--fix-n', '-o', str(ref))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return dict(dir=d, fq=str(fq), plain=str(plain), parts=str(parts), ref=ref.read_bytes(), line=_summary(r.stderr), set=f, bytes=want_set)


def _joined(out):
    parts = sorted(glob.glob(out + '.rank*'))
    assert len(parts) == RANKS, parts
    return b''.join(open(p, 'rb').read() for p in parts)


@pytest.mark.parametrize('which', ['plain', 'parts'])
def test_rank_files_are_the_one_process_bytes(fastq, tmp_path, which):
    out = str(tmp_path / 'out.fq')
    r = _ranks(['correct', '-f', fastq['fq'], '--fix-n', '--kmers-from', fastq[which], '-o', out])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == b'' and _joined(out) == fastq['ref']
    assert len(fastq['line']) == 1 and _summary(r.stderr) == [fastq['line'][0] + ' kmers_from=1 loaded_kmers=%d' % fastq['set']['n']]


def test_one_process_loads_the_set_without_torch(fastq, tmp_path):
    """The command as a process of its own: the bytes of the run that counted, the field at the end of its line, no torch."""
    code = ('import sys\nfrom kbbq import main\nmain.main(sys.argv[1:])\nsys.stdout.flush()\n'
            'sys.stderr.write("torch imported: %s\\n" % ("torch" in sys.modules))\n')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS', 'KBBQ_USE_TORCH')}
    env['PYTHONPATH'] = os.path.join(ROOT, 'kbbq-py_amd')
    out = str(tmp_path / 'out.fq')
    r = subprocess.run([sys.executable, '-c', code, 'correct', '-f', fastq['fq'], '--fix-n', '--kmers-from', fastq['parts'], '-o', out],
                       capture_output=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert 'torch imported: False' in r.stderr.decode()
    assert open(out, 'rb').read() == fastq['ref']
    assert _summary(r.stderr) == [fastq['line'][0] + ' kmers_from=1 loaded_kmers=%d' % fastq['set']['n']]


def test_a_corrupt_set_stops_every_rank(fastq, tmp_path):
    f = fastq['set']
    keys = f['keys'].copy()
    keys[[20, 21]] = keys[[21, 20]]
    bad = tmp_path / 'bad.set'
    bad.write_bytes(SM.retouch(fastq['bytes'], keys))
    out = str(tmp_path / 'out.fq')
    r = _ranks(['correct', '-f', fastq['fq'], '--kmers-from', str(bad), '-o', out], timeout=180)
    err = r.stderr.decode()
    assert r.returncode != 0 and glob.glob(out + '*') == []
    for j in range(RANKS):
        assert re.search(r'kbbq correct: rank %d: ValueError: k-mer set .*bad\.set: pair 21: ' % j, err), err[-3000:]
