"""`kbbq recalibrate -c reads.fq --skip-unresolved` on the MI355X against three existing commands, each run as the command line
runs, in a child process.  The expectation needs no tally model of its own: K1 leaves a base of quality below 6 out of every
table by the base's own quality alone, so the tally that skips the unresolved bases IS the tally of a file whose unresolved
bases (class 2 of the CPU model, tests/kmer_passes_model.py) have the quality character '!':

    kbbq correct -f reads.fq -o cor.fq [opts]
    kbbq recalibrate -f masked.fq cor.fq -g m.txt            saves the model of the masked tally
    kbbq recalibrate -f reads.fq cor.fq -g m.txt > want.fq   loads it: the qualities as read, recalibrated by that model
    kbbq recalibrate -c reads.fq --skip-unresolved [opts] -g m2.txt > got.fq

got.fq == want.fq and m2.txt == m.txt byte for byte, skipped_bases is the model's number of 2s and changed_bases correct's."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M
import kmer_passes_model as PM
from kmer_skip_model import masked_quals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_SEQUENTIAL', 'KBBQ_USE_TORCH', 'KBBQ_DEVICE_BUDGET'):
    ENV.pop(_var, None)

_memo = {}


def _kbbq(*argv, timeout=600):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + [str(a) for a in argv], capture_output=True, timeout=timeout, env=ENV)


def _ok(*argv):
    r = _kbbq(*argv)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r


def _text(names, seq, qual, meta):
    lens = np.asarray(meta, dtype=np.int64) & 0xFFFF
    return ''.join('@%s\n%s\n+\n%s\n' % (names[i], seq[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                   for i in range(seq.shape[0])).encode()


def _reads(name):
    """(seq, meta, qual) of a fixture, made once and left unchanged.  'pairs': 1800 reads of 100 bases; 'mixed': 36..300 bases,
    shortest first (recalibrate takes reads of non-decreasing length: several length bands)."""
    if name not in _memo:
        if name == 'pairs':
            seq, meta = M.synth(5, genome_len=6000, depth=30, err=0.01, len_lo=100, len_hi=100)[:2]
        else:
            seq, meta = M.synth(7, genome_len=8000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
            order = np.argsort(meta, kind='stable')
            seq, meta = seq[order], meta[order]
        qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
        for a in (seq, meta, qual):
            a.setflags(write=False)
        _memo[name] = (seq, meta, qual)
    return _memo[name]


def _classes(name, k=31, t=None, passes=1, fix_n=False):
    """(class plane, t) of the CPU model for a fixture, computed once per case."""
    key = (name, k, t, passes, fix_n)
    if key not in _memo:
        seq, meta, _ = _reads(name)
        solid, tt = PM.solid_set(seq, meta, k, t)
        cls = PM.passes(seq, meta, k, tt, passes, fix_n=fix_n, solid_keys=solid)[2]
        cls.setflags(write=False)
        _memo[key] = (cls, tt)
    return _memo[key]


def _figures(stderr, command):
    lines = [x for x in stderr.decode().splitlines() if x.startswith('kbbq %s:' % command)]
    assert len(lines) == 1, stderr.decode()
    m = re.match(r'kbbq %s: k=(\d+) min_count=(\d+) reads=(\d+) changed_bases=(\d+)(.*)$' % command, lines[0])
    assert m, lines[0]
    return tuple(int(x) for x in m.groups()[:4]), m.group(5)


def _observations(report):
    from kbbq import recaltable
    return int(recaltable.RecalibrationReport.fromfile(str(report)).tables[2].data['Observations'].sum())


def _case(d, name, names, kopts=(), ropts=(), model=None):
    """The four commands of the module's docstring in directory `d`; returns what the further assertions of a test need."""
    seq, meta, qual = _reads(name)
    cls, t = _classes(name, **(model or {}))
    inside = np.arange(seq.shape[1])[None, :] < (meta.astype(np.int64) & 0xFFFF)[:, None]
    assert not (cls[~inside] == 2).any()
    twos = int((cls == 2).sum())
    reads, masked, cor, m, m2 = (d / x for x in ('reads.fq', 'masked.fq', 'cor.fq', 'm.txt', 'm2.txt'))
    reads.write_bytes(_text(names, seq, qual, meta))
    masked.write_bytes(_text(names, seq, masked_quals(qual, cls), meta))
    c = _ok('correct', '-f', reads, '-o', cor, *kopts)
    (ck, ct, cn, changed), cextra = _figures(c.stderr, 'correct')
    assert ct == t and changed > 0
    _ok('recalibrate', '-f', masked, cor, '-g', m, *ropts)
    want = _ok('recalibrate', '-f', reads, cor, '-g', m, *ropts).stdout
    got = _ok('recalibrate', '-c', reads, '--skip-unresolved', '-g', m2, *kopts, *ropts)
    figures, extra = _figures(got.stderr, 'recalibrate')
    print('%s %s: class-2 bases %d of %d, changed %d' % (name, ' '.join(map(str, kopts)), twos, int(inside.sum()), changed))
    assert figures == (ck, ct, cn, changed)
    found = re.match(r' skipped_bases=(\d+)( fix_n=1)?( passes=\d+)?( prefilter=1 admitted=\d+ slots=\d+)?$', extra)
    assert found, extra                                      # directly after changed_bases, before fix_n
    assert int(found.group(1)) == twos
    # ... and the rest is what `correct` says (but for the prefilter's own figures: the order of the filter's atomics and the
    # table beside the resident reads decide them)
    pre = re.compile(r' prefilter=1 admitted=\d+ slots=\d+$')
    assert bool(pre.search(extra)) == bool(pre.search(cextra)) == ('--prefilter' in kopts)
    assert pre.sub('', extra) == ' skipped_bases=%d' % twos + pre.sub('', cextra)
    assert len(want) > 0 and got.stdout == want
    assert m2.read_bytes() == m.read_bytes() and len(m.read_bytes()) > 0
    return dict(reads=reads, cor=cor, m=m, twos=twos, bases=int(inside.sum()), cls=cls, qual=qual, got=got.stdout, figures=figures,
                counted=int(((cls == 2) & inside & (qual >= 33 + 6)).sum()))


def _pair_names(n):
    return ['r%d/%d' % (i >> 1, (i & 1) + 1) for i in range(n)]


def test_pairs_of_100_bases_and_what_the_option_changes(tmp_path):
    """Mate-pair rows at k = 31.  Guards: the class-2 share is at least 0.02 (the model gives 0.1135).  The report differs from
    the one of the command without the option, whose Observations are higher by the class-2 bases of quality 6 and above; and
    without the option stdout and stderr are those of the two commands, as before."""
    n = _reads('pairs')[0].shape[0]
    res = _case(tmp_path, 'pairs', _pair_names(n))
    assert res['twos'] >= 0.02 * res['bases']
    plain_report = tmp_path / 'plain.txt'
    two = _ok('recalibrate', '-f', res['reads'], res['cor'])
    plain = _ok('recalibrate', '-c', res['reads'], '-g', plain_report)
    assert plain.stdout == two.stdout and plain.stdout != res['got']
    figures, extra = _figures(plain.stderr, 'recalibrate')
    assert figures == res['figures'] and extra == ''
    assert plain_report.read_bytes() != res['m'].read_bytes()
    assert res['counted'] > 0 and _observations(plain_report) - _observations(res['m']) == res['counted']


def test_single_end_reads_in_twin_rows(tmp_path):
    n = _reads('pairs')[0].shape[0]
    _case(tmp_path, 'pairs', ['s%d' % i for i in range(n)])


def test_mixed_lengths_several_bands(tmp_path):
    from kbbq import fastx
    seq, meta, _ = _reads('mixed')
    assert len(fastx.length_bands(meta)) >= 4
    res = _case(tmp_path, 'mixed', ['r%d' % i for i in range(seq.shape[0])])
    assert res['twos'] >= 0.02 * res['bases']               # the model gives 0.0868


def test_infer_rg_with_three_read_groups(tmp_path):
    n = _reads('mixed')[0].shape[0]
    rng = np.random.default_rng(8)
    names = ['r%d_RG:Z:g%d' % (i, g) for i, g in enumerate(rng.integers(0, 3, n))]
    res = _case(tmp_path, 'mixed', names, ropts=('--infer-rg',))
    one_group = _ok('recalibrate', '-c', res['reads'], '--skip-unresolved')
    assert one_group.stdout != res['got']                    # the read groups matter


def test_fix_n(tmp_path):
    seq = _reads('mixed')[0]
    assert (seq == PM.NCH).any()
    res = _case(tmp_path, 'mixed', ['r%d' % i for i in range(seq.shape[0])], kopts=('--fix-n',), model=dict(fix_n=True))
    assert res['figures'][3] > int((_classes('mixed')[0] == 1).sum())       # the N rule fixes something


def test_three_passes(tmp_path):
    n = _reads('mixed')[0].shape[0]
    res = _case(tmp_path, 'mixed', ['r%d' % i for i in range(n)], kopts=('--passes', '3'), model=dict(passes=3))
    assert 0 < res['twos'] < int((_classes('mixed')[0] == 2).sum())         # above 0, and fewer than after one pass


def test_prefilter(tmp_path):
    n = _reads('mixed')[0].shape[0]
    _case(tmp_path, 'mixed', ['r%d' % i for i in range(n)], kopts=('--prefilter',))


def test_k_and_min_count(tmp_path):
    n = _reads('mixed')[0].shape[0]
    res = _case(tmp_path, 'mixed', ['r%d' % i for i in range(n)], kopts=('-k', '21', '--min-count', '3'), model=dict(k=21, t=3))
    assert res['figures'][:2] == (21, 3) and res['twos'] > 0


def test_a_band_redone_in_character_rows_raises_what_the_two_file_form_raises(tmp_path):
    """A quality above 42 makes the tally refuse the band's layout: the band is redone one character row per read, its tally plane
    made by the character form of the call, and the row-per-read kernel reports the read as it does for the two-file form."""
    seq, meta, qual = _reads('mixed')
    qual = qual.copy()
    qual[seq.shape[0] // 2, 5] = 33 + 43
    fq = tmp_path / 'q43.fq'
    fq.write_bytes(_text(['r%d' % i for i in range(seq.shape[0])], seq, qual, meta))
    two = _kbbq('recalibrate', '-f', fq, fq)
    one = _kbbq('recalibrate', '-c', fq, '--skip-unresolved')
    assert two.returncode != 0 and one.returncode != 0 and one.stdout == b''

    def raised(r):
        last = [x for x in r.stderr.decode().splitlines() if re.match(r'[A-Za-z_.]*(Error|Exception)\b', x)][-1]
        return last.split(':')[0]
    assert raised(one) == raised(two) == 'IndexError'


def test_a_band_redone_in_character_rows_tallies_the_same(tmp_path, monkeypatch):
    """The fallback with input it accepts, in process: every band's own layout is refused by a stand-in for K1's launcher, so each
    band is redone one character row per read and its tally plane comes from the character form of the call.  Output, report and
    skipped_bases are those of the run whose bands were tallied in their layouts, and not those of the run without the option."""
    from kbbq import _device as dev
    from kbbq import recalibrate
    seq, meta, qual = _reads('mixed')
    cls, _ = _classes('mixed')
    fq = tmp_path / 'reads.fq'
    fq.write_bytes(_text(['r%d' % i for i in range(seq.shape[0])], seq, qual, meta))

    def run(tag, **kw):
        out, report = tmp_path / (tag + '.fq'), tmp_path / (tag + '.txt')
        info = recalibrate.recalibrate_corrected(str(fq), output=str(out), gatkreport=str(report), **kw)
        return info, out.read_bytes(), report.read_bytes()
    laid = run('laid', skip_unresolved=True)
    plain = run('plain')
    refused = []
    real = dev.accumulate

    def accumulate(batch, *args, **kw):
        if batch.nib or isinstance(batch, dev.PairBatch) or batch.seg is not None:
            refused.append(batch.layout_key())
            raise ValueError('a layout the tally does not serve (the test says so)')
        assert batch.tally_qual is None                      # the plane has taken the place of batch.qual by now
        return real(batch, *args, **kw)

    def accumulate_bands(*args, **kw):
        raise ValueError('no merged launch (the test says so)')
    monkeypatch.setattr(dev, 'accumulate', accumulate)
    monkeypatch.setattr(dev, 'accumulate_bands', accumulate_bands)
    redone = run('redone', skip_unresolved=True)
    assert len(refused) >= 4                                 # every length band went the other way
    assert redone[1] == laid[1] and redone[2] == laid[2] and len(laid[1]) > 0
    assert redone[0]['skipped_bases'] == laid[0]['skipped_bases'] == int((cls == 2).sum()) > 0
    assert redone[0]['changed_bases'] == laid[0]['changed_bases'] == plain[0]['changed_bases']
    assert plain[2] != laid[2] and 'skipped_bases' not in plain[0]


def test_refused_as_before(tmp_path):
    """Everything -c refuses stays refused with the option: an existing report, a device budget the reads do not fit."""
    seq, meta, qual = _reads('mixed')
    fq = tmp_path / 'reads.fq'
    fq.write_bytes(_text(['r%d' % i for i in range(seq.shape[0])], seq, qual, meta))
    report = tmp_path / 'old.txt'
    report.write_text('x')
    r = _kbbq('recalibrate', '-c', fq, '--skip-unresolved', '-g', report)
    assert r.returncode != 0 and b'ValueError' in r.stderr and r.stdout == b''
    env = dict(ENV, KBBQ_DEVICE_BUDGET='1M')
    r = subprocess.run([sys.executable, '-m', 'kbbq.main', 'recalibrate', '-c', str(fq), '--skip-unresolved'], capture_output=True,
                       timeout=600, env=env)
    assert r.returncode != 0 and b'kbbq correct -f' in r.stderr and r.stdout == b''
