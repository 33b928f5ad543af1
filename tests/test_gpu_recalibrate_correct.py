"""`kbbq recalibrate -c reads.fq` on the MI355X against the two commands it replaces -- `kbbq correct -f reads.fq -o cor.fq`, then
`kbbq recalibrate -f reads.fq cor.fq` --, each run as the command line runs, in a child process: the same bytes on stdout, the same
threshold and number of changed bases on stderr, the same report."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_SEQUENTIAL', 'KBBQ_USE_TORCH'):
    ENV.pop(_var, None)


def _kbbq(*argv, timeout=600):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + [str(a) for a in argv], capture_output=True, timeout=timeout, env=ENV)


def _write(path, names, seq, meta, seed=3, qual=None):
    lens = np.asarray(meta, dtype=np.int64) & 0xFFFF
    if qual is None:
        qual = (np.random.default_rng(seed).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    text = ''.join('@%s\n%s\n+\n%s\n' % (names[i], seq[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                   for i in range(seq.shape[0]))
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(path, 'wb') as fh:
        fh.write(text.encode())
    return str(path)


def _mixed():
    seq, meta = M.synth(7, genome_len=8000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
    order = np.argsort(meta, kind='stable')                  # recalibrate takes reads of non-decreasing length
    return seq[order], meta[order]


def _one_length(S, seed):
    seq, meta = M.synth(seed, genome_len=6000, depth=30, err=0.01, len_lo=S, len_hi=S)[:2]
    n = seq.shape[0] & ~1
    return seq[:n], meta[:n]


def _figures(stderr, command):
    lines = [x for x in stderr.decode().splitlines() if x.startswith('kbbq %s:' % command)]
    assert len(lines) == 1, stderr.decode()
    m = re.match(r'kbbq %s: k=(\d+) min_count=(\d+) reads=(\d+) changed_bases=(\d+)(.*)$' % command, lines[0])
    assert m, lines[0]
    return tuple(int(x) for x in m.groups()[:4]), m.group(5)


def _two_commands(fq, tmp_path, kopts=(), ropts=()):
    """(stdout of recalibrate -f fq cor.fq, correct's figures)"""
    cor = tmp_path / 'two.cor.fq'
    c = _kbbq('correct', '-f', fq, '-o', cor, *kopts)
    assert c.returncode == 0, c.stderr.decode()
    r = _kbbq('recalibrate', '-f', fq, cor, *ropts)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout, _figures(c.stderr, 'correct')


def _same(fq, tmp_path, kopts=(), ropts=()):
    want, (figures, extra) = _two_commands(fq, tmp_path, kopts, ropts)
    r = _kbbq('recalibrate', '-c', fq, *kopts, *ropts)
    assert r.returncode == 0, r.stderr.decode()
    got, gextra = _figures(r.stderr, 'recalibrate')
    assert got == figures and got[3] > 0
    assert r.stdout == want and len(want) > 0
    return r, extra, gextra


@pytest.fixture(scope='module')
def mixed_fq(tmp_path_factory):
    seq, meta = _mixed()
    d = tmp_path_factory.mktemp('mixed')
    names = ['r%d' % i for i in range(seq.shape[0])]
    return _write(d / 'reads.fq', names, seq, meta), _write(d / 'reads.fq.gz', names, seq, meta), seq, meta


def test_mixed_lengths_several_bands(mixed_fq, tmp_path):
    fq, _, seq, meta = mixed_fq
    from kbbq import fastx
    assert len(fastx.length_bands(meta)) >= 4
    _same(fq, tmp_path)


def test_mixed_lengths_gz(mixed_fq, tmp_path):
    fq, gz, _, _ = mixed_fq
    r, _, _ = _same(gz, tmp_path)
    plain = _kbbq('recalibrate', '-c', fq)
    assert plain.returncode == 0 and plain.stdout == r.stdout


def test_paired_reads_of_one_length(tmp_path):
    seq, meta = _one_length(100, 21)
    names = ['r%d/%d' % (i >> 1, (i & 1) + 1) for i in range(seq.shape[0])]
    fq = _write(tmp_path / 'pairs.fq', names, seq, meta)
    env = dict(ENV, KBBQ_TIMING='1')
    _same(fq, tmp_path)
    r = subprocess.run([sys.executable, '-m', 'kbbq.main', 'recalibrate', '-c', fq], capture_output=True, timeout=600, env=env)
    assert r.returncode == 0 and b'k-mer count' in r.stderr and b'k-mer correct' in r.stderr


def test_single_end_reads_of_one_length(tmp_path):
    seq, meta = _one_length(100, 22)
    fq = _write(tmp_path / 'single.fq', ['s%d' % i for i in range(seq.shape[0] - 1)], seq[:-1], meta[:-1])
    _same(fq, tmp_path)


def test_infer_rg_with_three_read_groups(mixed_fq, tmp_path):
    _, _, seq, meta = mixed_fq
    rng = np.random.default_rng(8)
    names = ['r%d_RG:Z:g%d' % (i, g) for i, g in enumerate(rng.integers(0, 3, seq.shape[0]))]
    fq = _write(tmp_path / 'rg.fq', names, seq, meta)
    r, _, _ = _same(fq, tmp_path, ropts=('--infer-rg',))
    plain = _kbbq('recalibrate', '-c', fq)
    assert plain.returncode == 0 and plain.stdout != r.stdout          # the read groups matter


def test_prefilter(mixed_fq, tmp_path):
    fq = mixed_fq[0]
    r, extra, gextra = _same(fq, tmp_path, kopts=('--prefilter',))
    assert re.match(r' prefilter=1 admitted=\d+ slots=\d+$', gextra) and re.match(r' prefilter=1 admitted=\d+ slots=\d+$', extra)
    plain = _kbbq('recalibrate', '-c', fq)
    assert plain.stdout == r.stdout and b'prefilter' not in plain.stderr


def test_k_and_min_count(mixed_fq, tmp_path):
    r, _, _ = _same(mixed_fq[0], tmp_path, kopts=('-k', '21', '--min-count', '3'))
    assert _figures(r.stderr, 'recalibrate')[0][:2] == (21, 3)


def test_output_file(mixed_fq, tmp_path):
    fq = mixed_fq[0]
    want, _ = _two_commands(fq, tmp_path)
    out = tmp_path / 'out.fq'
    r = _kbbq('recalibrate', '-c', fq, '-o', out)
    assert r.returncode == 0 and r.stdout == b'' and out.read_bytes() == want


def test_new_report_equals_the_two_commands(mixed_fq, tmp_path):
    fq = mixed_fq[0]
    a, b = tmp_path / 'two.grp', tmp_path / 'one.grp'
    want, _ = _two_commands(fq, tmp_path, ropts=('-g', a))
    r = _kbbq('recalibrate', '-c', fq, '-g', b)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want and b.read_bytes() == a.read_bytes() and len(a.read_bytes()) > 0
    again = _kbbq('recalibrate', '-c', fq, '-g', b)                     # the report exists now
    assert again.returncode != 0 and b'ValueError' in again.stderr and again.stdout == b''


def test_a_table_that_does_not_fit_names_the_options(mixed_fq):
    r = _kbbq('recalibrate', '-c', mixed_fq[0], '--slots', '1024')
    assert r.returncode != 0 and r.stdout == b''
    assert b'KmerTableFull' in r.stderr and b'--slots' in r.stderr and b'--prefilter' in r.stderr


def test_empty_file(tmp_path):
    fq = tmp_path / 'empty.fq'
    fq.write_bytes(b'')
    r = _kbbq('recalibrate', '-c', fq)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b''
    assert _figures(r.stderr, 'recalibrate')[0][2:] == (0, 0)


def test_quality_above_42_raises_what_the_two_file_form_raises(mixed_fq, tmp_path):
    _, _, seq, meta = mixed_fq
    qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    qual[seq.shape[0] // 2, 5] = 33 + 43
    fq = _write(tmp_path / 'q43.fq', ['r%d' % i for i in range(seq.shape[0])], seq, meta, qual=qual)
    two = _kbbq('recalibrate', '-f', fq, fq)
    one = _kbbq('recalibrate', '-c', fq)
    assert two.returncode != 0 and one.returncode != 0

    def raised(r):
        last = [x for x in r.stderr.decode().splitlines() if re.match(r'[A-Za-z_.]*(Error|Exception)\b', x)][-1]
        return last.split(':')[0]
    assert raised(one) == raised(two) == 'IndexError'


def test_the_command_does_not_import_torch(mixed_fq, tmp_path):
    out = tmp_path / 'out.fq'
    code = ('import sys\nfrom kbbq import main\nmain.main(["recalibrate", "-c", %r, "-o", %r])\n'
            'assert "torch" not in sys.modules, "torch was imported"\nprint("no torch")\n' % (mixed_fq[0], str(out)))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b'no torch\n' and out.stat().st_size > 0


def test_in_process_info_equals_the_model(mixed_fq, tmp_path):
    from kbbq import recalibrate
    fq, _, seq, meta = mixed_fq
    want, changed, t = M.correct(seq, meta, 31)
    keys, counts = M.count(seq, meta, 31)
    out = tmp_path / 'out.fq'
    info = recalibrate.recalibrate_corrected(fq, output=str(out))
    assert info['k'] == 31 and info['min_count'] == t and info['reads'] == seq.shape[0]
    assert info['changed_bases'] == int(changed.sum()) > 0
    assert np.array_equal(info['hist'], M.histogram(counts)) and info['slots'] >= 2 * keys.size and 'admitted' not in info
    text = out.read_text().splitlines()
    assert len(text) == 4 * seq.shape[0]
    lens = meta.astype(np.int64)
    assert text[1::4] == [seq[i, :lens[i]].tobytes().decode() for i in range(seq.shape[0])]      # the reads as read, not corrected
    pre = recalibrate.recalibrate_corrected(fq, output=str(tmp_path / 'pre.fq'), prefilter=True)
    assert pre['changed_bases'] == info['changed_bases'] and 0 < pre['admitted'] < keys.size and pre['slots'] < info['slots']
    assert (tmp_path / 'pre.fq').read_bytes() == out.read_bytes()
    with pytest.raises(ValueError, match='kbbq correct -f'):
        os.environ['KBBQ_DEVICE_BUDGET'] = '1M'
        try:
            recalibrate.recalibrate_corrected(fq, output=str(tmp_path / 'no.fq'))
        finally:
            del os.environ['KBBQ_DEVICE_BUDGET']
