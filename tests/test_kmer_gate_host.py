"""`--kmer-min-qual Q` without a GPU: the CPU model's own properties (tests/kmer_gate_model.py) and the figures of its two
fixtures, kbbq.kmer.check_kmer_min_qual, every argparse refusal of the five commands, the option's way down to the calls only
when it is given, the place of ` kmer_min_qual=Q counted_windows=N` in each stderr line, and the symbol in the header, the
library and the prototypes."""
import os
import re

import numpy as np
import pytest

import kmer_gate_model as G
import kmer_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize('name, figures', (('F1', dict(keys=(27967, 12995), t=(3, 2), differ=28)),
                                           ('F2', dict(keys=(35606, 24004), t=(4, 3), differ=1, windows=(120936, 74515)))))
def test_the_fixtures_are_the_ones_the_figures_are_of(name, figures):
    f = G.fixture(name)
    G.assert_not_vacuous(f)
    assert (f['plain_keys'].size, f['keys'].size) == figures['keys'] and (f['plain_t'], f['t']) == figures['t']
    assert int((f['out'] != f['plain_out']).sum()) == figures['differ']
    if 'windows' in figures:
        assert (f['plain_windows'], f['windows']) == figures['windows']
    # the counted windows are the sum of the counts, and the histogram and the threshold are the gated table's
    assert f['windows'] == int(f['counts'].sum()) == int(M.windows(f['gated'], f['meta'], f['k'])[2].sum())
    assert np.array_equal(f['hist'], M.histogram(f['counts'])) and f['t'] == M.threshold(f['hist'])
    # gate(): 'N' exactly where the quality byte is below Q + 33, every other byte as read
    low = f['qual'] < f['Q'] + 33
    assert (f['gated'][low] == ord('N')).all() and np.array_equal(f['gated'][~low], f['seq'][~low])
    # the correction runs on the rows as read: a gated base may be changed, and one was
    changed = f['out'] != f['seq']
    assert (changed & low).any() and not changed[f['seq'] == ord('N')].any()
    # the classes of the rule against the gated solid set say the same
    cls, t = G.classify(f['seq'], f['qual'], f['meta'], f['k'], f['Q'] + 33)
    assert t == f['t'] and np.array_equal(cls == 1, changed)


def test_a_q_below_every_quality_present_is_no_gate():
    f = G.fixture('F2')
    lens = f['meta'].astype(np.int64)
    inside = np.arange(f['seq'].shape[1])[None, :] < lens[:, None]
    lowest = int(f['qual'][inside].min())
    assert lowest == 2 + 33
    assert np.array_equal(G.gate(f['seq'], f['qual'], lowest), f['seq'])          # (the padding is 'N' already)
    keys, counts = G.count(f['seq'], f['qual'], f['meta'], f['k'], lowest)
    assert np.array_equal(keys, f['plain_keys']) and int(counts.sum()) == f['plain_windows']
    assert G.counted_windows(f['seq'], f['qual'], f['meta'], f['k'], lowest) == f['plain_windows']
    # ... and one above it gates something
    assert G.counted_windows(f['seq'], f['qual'], f['meta'], f['k'], lowest + 1) < f['plain_windows']
    # a gate that leaves nothing leaves no window
    assert G.counted_windows(f['seq'], f['qual'], f['meta'], f['k'], 93 + 33) == 0


# ---------------------------------------------------------------- check_kmer_min_qual
def test_check_kmer_min_qual():
    from kbbq import kmer
    assert kmer.check_kmer_min_qual(None) is None and kmer.check_kmer_min_qual(None, False) is None
    for good in (1, 20, 93, np.int64(24), 7.0):
        assert kmer.check_kmer_min_qual(good) == int(good) and type(kmer.check_kmer_min_qual(good)) is int
    for bad in (0, 94, -1, 2.5, True, '20', b'20', [20], float('nan')):
        with pytest.raises(ValueError, match=r'kmer_min_qual must be an integer in 1\.\.93'):
            kmer.check_kmer_min_qual(bad)
    with pytest.raises(ValueError, match='needs the qualities'):
        kmer.check_kmer_min_qual(20, False)
    assert kmer.min_qual_field({}) == '' and kmer.min_qual_field(dict(kmer_min_qual=None)) == ''
    assert kmer.min_qual_field(dict(kmer_min_qual=20, counted_windows=7)) == ' kmer_min_qual=20 counted_windows=7'


def _never(*a, **kw):
    raise AssertionError('a device call')


def test_python_refuses_before_any_device_call(monkeypatch):
    from kbbq import _native, benchmark, kmer, recalibrate
    from kbbq.gatk import bqsr
    monkeypatch.setattr(_native, 'load', _never)
    monkeypatch.setattr(kmer, '_ctx', _never)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    seq, meta = np.full((2, 48), ord('A'), dtype=np.uint8), np.array([40, 40], dtype=np.uint32)
    qual = np.full((2, 48), 70, dtype=np.uint8)
    with pytest.raises(ValueError, match=r'1\.\.93'):
        kmer.correct_reads(seq, meta, qual_plane=qual, kmer_min_qual=0)
    with pytest.raises(ValueError, match='needs the qualities'):
        kmer.correct_reads(seq, meta, kmer_min_qual=20)
    with pytest.raises(ValueError, match='needs the qualities'):
        kmer.gate_plane(seq, None, meta, 31, 20)
    for call in (lambda: kmer.correct_fastq('x.fq', 'y.fq', kmer_min_qual=94), lambda: kmer.main_correct('x.fq', kmer_min_qual=94),
                 lambda: kmer.correct_fastq_ranks('x.fq', 'y.fq', kmer_min_qual=94),
                 lambda: recalibrate.recalibrate_corrected('x.fq', kmer_min_qual=94),
                 lambda: bqsr.bam_to_kmer_covariates('x.sam', kmer_min_qual=94),
                 lambda: benchmark.benchmark_kmers('x.sam', {}, {}, kmer_min_qual=94)):
        with pytest.raises(ValueError, match=r'kmer_min_qual must be an integer in 1\.\.93, got 94'):
            call()
    with pytest.raises(ValueError, match=r'recalibrate -b --kmers: kmer_min_qual must be an integer in 1\.\.93, got 0'):
        recalibrate.check_bam_kmers('x.sam', kmer_min_qual=0)


# ---------------------------------------------------------------- command line
def _no_ranks(monkeypatch):
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the commands then leave the memory back end alone


COMMANDS = (['correct', '-f', 'x.fq'], ['recalibrate', '-c', 'x.fq'], ['recalibrate', '-b', 'x.sam', '--kmers'],
            ['bqsr', '-b', 'x', '--kmers', '-g', 'r'], ['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '--kmers'])


@pytest.mark.parametrize('command', COMMANDS, ids=lambda c: '-'.join(c[:2] + c[3:4]))
@pytest.mark.parametrize('value', ('0', '94', '-1', 'twenty', '2.5', ''))
def test_values_outside_the_range_are_argparse_errors(monkeypatch, capsys, command, value):
    from kbbq import main, parallel
    _no_ranks(monkeypatch)
    monkeypatch.setattr(parallel, 'init_from_env', _never)              # before the ranks join
    with pytest.raises(SystemExit) as exc:
        main.main(command + ['--kmer-min-qual', value])
    assert exc.value.code == 2
    assert 'argument --kmer-min-qual' in capsys.readouterr().err


@pytest.mark.parametrize('argv, message', (
    (['recalibrate', '-f', 'a.fq', 'b.fq', '--kmer-min-qual', '20'], '--kmer-min-qual: only with -c/--correct or with -b --kmers'),
    (['recalibrate', '-b', 'a.bam', '--kmer-min-qual', '20'], '--kmer-min-qual: only with -c/--correct or with -b --kmers'),
    (['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--kmer-min-qual', '20'], '--kmer-min-qual: only with --kmers'),
    (['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '--kmer-min-qual', '20'], '--kmer-min-qual: only with --kmers'),
))
def test_the_option_only_with_the_k_mer_form(monkeypatch, capsys, argv, message):
    from kbbq import benchmark as bm, main, parallel, recalibrate as recal
    from kbbq.gatk import bqsr
    _no_ranks(monkeypatch)
    monkeypatch.setattr(parallel, 'init_from_env', _never)
    monkeypatch.setattr(recal, 'recalibrate', lambda **kw: pytest.fail('ran'))
    monkeypatch.setattr(bm, 'benchmark', lambda **kw: pytest.fail('ran'))
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: pytest.fail('ran'))
    with pytest.raises(SystemExit) as exc:
        main.main(argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


class _Report:
    def write(self, path):
        pass


def test_the_option_reaches_the_commands_only_when_given_and_the_field_has_its_place(monkeypatch, capsys):
    from kbbq import aln, benchmark as bm, kmer, main, recalibrate as recal
    from kbbq.gatk import bqsr
    _no_ranks(monkeypatch)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    seen = []
    gate = ['--kmer-min-qual', '20']
    rest = ['--passes', '2', '--partitions', '3', '--prefilter']

    def gated(info, kw):
        if kw.get('kmer_min_qual') is not None:
            info.update(kmer_min_qual=kw['kmer_min_qual'], counted_windows=41, windows=99)
        if kw.get('partitions', 1) != 1:
            info.update(partitions=kw['partitions'])
        return info

    # correct: main.correct -> kmer.main_correct -> kmer.correct_fastq
    def correct_fastq(path, out, **kw):
        seen.append(kw)
        return gated(dict(k=kw['k'], min_count=4, reads=9, changed=np.array([1, 2]), admitted=5, slots=32), kw)
    monkeypatch.setattr(kmer, 'correct_fastq', correct_fastq)
    for more in ([], gate, gate + rest + ['--fix-n']):
        main.main(['correct', '-f', 'x.fq'] + more)
    assert 'kmer_min_qual' not in seen[0] and seen[1]['kmer_min_qual'] == seen[2]['kmer_min_qual'] == 20
    assert capsys.readouterr().err.splitlines() == [
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 kmer_min_qual=20 counted_windows=41',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 fix_n=1 passes=2 partitions=3 kmer_min_qual=20 counted_windows=41 '
        'prefilter=1 admitted=5 slots=32']

    # recalibrate -c
    del seen[:]
    monkeypatch.setattr(recal, 'check_corrected', lambda *a, **kw: None)
    monkeypatch.setattr(recal, 'recalibrate_corrected', lambda path, **kw: seen.append(kw) or gated(
        dict(k=kw['k'], min_count=3, reads=5, changed_bases=7, admitted=11, slots=16, skipped_bases=2), kw))
    for more in ([], gate, gate + rest + ['--skip-unresolved', '--fix-n']):
        main.main(['recalibrate', '-c', 'x.fq'] + more)
    assert 'kmer_min_qual' not in seen[0] and seen[1]['kmer_min_qual'] == seen[2]['kmer_min_qual'] == 20
    assert [x for x in capsys.readouterr().err.splitlines() if x.startswith('kbbq ')] == [
        'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7',
        'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 kmer_min_qual=20 counted_windows=41',
        'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 skipped_bases=2 fix_n=1 passes=2 partitions=3 kmer_min_qual=20 '
        'counted_windows=41 prefilter=1 admitted=11 slots=16']

    # bqsr --kmers
    del seen[:]

    def kmers(bam, **kw):
        seen.append(kw)
        gated(kw['info'], kw).update(k=kw['k'], min_count=7, reads=5, flagged_bases=11, admitted=13, slots=1024, skipped_bases=17)
        return _Report()
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: 'opened:' + p)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', kmers)
    for more in ([], gate, gate + rest + ['--skip-unresolved']):
        main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp'] + more)
    assert 'kmer_min_qual' not in seen[0] and seen[1]['kmer_min_qual'] == seen[2]['kmer_min_qual'] == 20
    assert capsys.readouterr().err.splitlines() == [
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11',
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11 kmer_min_qual=20 counted_windows=41',
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11 skipped_bases=17 passes=2 partitions=3 kmer_min_qual=20 counted_windows=41 '
        'prefilter=1 admitted=13 slots=1024']

    # recalibrate -b --kmers
    del seen[:]
    checked = []
    monkeypatch.setattr(recal, 'check_bam_kmers', lambda *a, **kw: checked.append(kw))
    monkeypatch.setattr(recal, 'check_bam_records', lambda *a, **kw: None)
    monkeypatch.setattr(recal, 'recalibrate_bam', lambda bam, **kw: seen.append(kw['kmers']) or gated(
        dict(k=kw['kmers']['k'], min_count=7, reads=5, flagged_bases=11, admitted=13, slots=1024, skipped_bases=17), kw['kmers']))
    for more in ([], gate, gate + rest + ['--skip-unresolved']):
        main.main(['recalibrate', '-b', 'x.sam', '--kmers'] + more)
    assert 'kmer_min_qual' not in seen[0] and seen[1]['kmer_min_qual'] == seen[2]['kmer_min_qual'] == 20
    assert [x for x in capsys.readouterr().err.splitlines() if x.startswith('kbbq ')] == [
        'kbbq recalibrate: k=31 min_count=7 reads=5 flagged_bases=11',
        'kbbq recalibrate: k=31 min_count=7 reads=5 flagged_bases=11 kmer_min_qual=20 counted_windows=41',
        'kbbq recalibrate: k=31 min_count=7 reads=5 flagged_bases=11 skipped_bases=17 passes=2 partitions=3 kmer_min_qual=20 '
        'counted_windows=41 prefilter=1 admitted=13 slots=1024']

    # benchmark --kmers
    del seen[:]
    monkeypatch.setattr(bm, 'benchmark', lambda **kw: seen.append(kw))
    for more in ([], gate):
        main.main(['benchmark', '-b', 'x.sam', '-r', 'x.fa', '-v', 'x.vcf', '--kmers'] + more)
    assert 'kmer_min_qual' not in seen[0]['kmers'] and seen[1]['kmers'] == dict(seen[0]['kmers'], kmer_min_qual=20)
    info = dict(k=31, min_count=4, reads=9, bases=100, errors=10, flagged=8, flagged_errors=8, unresolved=5, unresolved_errors=1,
                prefilter=False, admitted=None, slots=64)
    line = bm.kmer_summary(info)
    assert bm.kmer_summary(dict(info, kmer_min_qual=None)) == line and 'kmer_min_qual' not in line
    assert bm.kmer_summary(dict(info, kmer_min_qual=20, counted_windows=41)) == line + ' kmer_min_qual=20 counted_windows=41'
    assert bm.kmer_summary(dict(info, passes=3, partitions=4, prefilter=True, admitted=7, kmer_min_qual=20, counted_windows=41)) \
        == line + ' passes=3 partitions=4 kmer_min_qual=20 counted_windows=41 prefilter=1 admitted=7 slots=64'


def test_the_keyword_goes_down_only_when_given(monkeypatch):
    from kbbq import kmer
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    seen = {}

    def fake(path, out, **kw):
        seen.update(kw=kw)
        return dict(k=kw['k'], min_count=4, reads=9, changed=np.array([1]))
    monkeypatch.setattr(kmer, 'correct_fastq', fake)
    kmer.main_correct('x.fq')
    assert 'kmer_min_qual' not in seen['kw']
    kmer.main_correct('x.fq', kmer_min_qual=20)
    assert seen['kw']['kmer_min_qual'] == 20
    assert kmer._min_qual_kw(None) == {} and kmer._min_qual_kw(None, qual_plane=1) == {}
    assert kmer._min_qual_kw(20, qual_plane=1) == dict(kmer_min_qual=20, qual_plane=1)


# ---------------------------------------------------------------- the C ABI
def test_the_symbol_is_exported_declared_and_prototyped():
    import ctypes
    from kbbq import _native as N
    lib = N.load()
    assert hasattr(lib, 'kbbq_kmer_gate_rows_dev')
    ret, args = N.PROTOTYPES['kbbq_kmer_gate_rows_dev']
    assert ret is ctypes.c_int and len(args) == 11
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    assert re.search(r'^int kbbq_kmer_gate_rows_dev\(kbbq_ctx\* ctx, const uint8_t\* d_seq, const uint8_t\* d_qual, const uint32_t\* d_meta, '
                     r'int64_t nrows,\s+int pitch, int flags, int k, int qual_byte_min, uint8_t\* d_out, uint64_t\* d_windows\);',
                     header, flags=re.M)
    assert 'counting d_out with any existing count call yields exactly *d_windows insertions' in re.sub(r'\s*\n \* ', ' ', header)
    assert not re.search(r'^int kbbq_kmer_gate\w*\((?!kbbq_ctx\* ctx, const uint8_t\* d_seq)', header, flags=re.M)     # no host-buffer form
    assert lib.kbbq_abi_version() == 1
    # refused on the arguments alone: no context exists without a device
    assert lib.kbbq_kmer_gate_rows_dev(None, None, None, None, 0, 16, 0, 31, 53, None, None) == N.KBBQ_E_ARG
