"""`kbbq recalibrate -b ALN --kmers`, host side, no GPU: the command line forwards every option, the stderr line is `bqsr --kmers`'s
under another prefix, what the one-run path refuses it refuses before any device call or collective (the records' refusals after
the one parse of the file, which is host work), the dispatcher keeps its NotImplementedError cases, and a report parsed from its
text is the report parsed from its file."""
import os

import numpy as np
import pytest

HEADER = ['@HD\tVN:1.6\tSO:unsorted', '@SQ\tSN:chr1\tLN:1000', '@RG\tID:g0\tPU:unit0\tSM:s', '@RG\tID:g1\tPU:unit1\tSM:s']


def _record(i, seq='ACGTACGTACGTACGTACGT', qual=None, rg='g0', oq=None):
    qual = 'I' * len(seq) if qual is None else qual
    tags = ([] if rg is None else ['RG:Z:%s' % rg]) + ([] if oq is None else ['OQ:Z:%s' % oq])
    return '\t'.join(['r%d' % i, '0', 'chr1', str(10 + i), '60', '%dM' % len(seq), '*', '0', '0', seq, qual] + tags)


def _sam(tmp_path, records, name='aln.sam'):
    p = tmp_path / name
    p.write_text('\n'.join(HEADER + records) + '\n')
    return str(p)


@pytest.fixture
def cli(monkeypatch):
    """main.main with every recalibrate path recorded instead of run."""
    from kbbq import aln, main, recalibrate
    calls = []
    monkeypatch.setattr(aln, 'AlignmentFile', lambda path: path)             # (the parse; the path stands for the parsed file)
    monkeypatch.setattr(recalibrate, 'check_bam_records', lambda *a, **kw: calls.append(('records', a, kw)))
    info = dict(k=15, min_count=4, reads=600, flagged_bases=77, slots=2048, prefilter=False, admitted=None)
    monkeypatch.setattr(recalibrate, 'recalibrate', lambda **kw: calls.append(('two', kw)))
    monkeypatch.setattr(recalibrate, 'recalibrate_corrected', lambda path, **kw: calls.append(('one', dict(kw, path=path))))
    monkeypatch.setattr(recalibrate, 'recalibrate_bam', lambda bam, **kw: calls.append(('bam', dict(kw, bam=bam))) or dict(info))
    monkeypatch.setattr(recalibrate, 'check_bam_kmers', lambda *a, **kw: calls.append(('check', a, kw)))
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                # the command then leaves the memory back end alone
    return main, calls, info


def test_the_parser_forwards_every_option(cli, capsys):
    main, calls, info = cli
    main.main(['recalibrate', '-b', 'x.sam', '--kmers'])
    assert calls[0] == ('check', ('x.sam', None, None, 31, None, False, 4), {})
    assert calls[1] == ('records', ('x.sam', False, 31, None, False, 4), {})
    assert calls[2] == ('bam', dict(bam='x.sam', use_oq=False, set_oq=False, gatkreport=None, output=None,
                                    kmers=dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4)))
    assert capsys.readouterr().err == 'kbbq recalibrate: k=15 min_count=4 reads=600 flagged_bases=77\n'
    del calls[:]
    info.update(skipped_bases=5, admitted=99)
    main.main(['recalibrate', '--bam', 'x.bam', '--kmers', '-k', '21', '--min-count', '3', '--slots', '4096', '--prefilter',
               '--filter-bits', '8', '--skip-unresolved', '--passes', '2', '--partitions', 'auto', '-u', '-s', '-g', 'm.grp', '-o', 'o.sam'])
    assert calls[0] == ('check', ('x.bam', 'm.grp', 'o.sam', 21, 3, True, 8), dict(partitions='auto', passes=2))
    assert calls[1] == ('records', ('x.bam', True, 21, 3, True, 8), {})
    assert calls[2] == ('bam', dict(bam='x.bam', use_oq=True, set_oq=True, gatkreport='m.grp', output='o.sam',
                                    kmers=dict(k=21, min_count=3, slots=4096, prefilter=True, filter_bits=8, skip_unresolved=True,
                                               passes=2, partitions='auto')))
    del calls[:]
    main.main(['recalibrate', '-b', 'x.sam', '--kmers', '--partitions', '3'])
    assert calls[0][2] == dict(partitions=3) and calls[2][1]['kmers']['partitions'] == 3 and 'passes' not in calls[2][1]['kmers']
    capsys.readouterr()


def test_without_kmers_the_call_is_the_one_it_was(cli, capsys):
    main, calls, _ = cli
    main.main(['recalibrate', '-b', 'x.bam', '-u', '-s'])
    assert calls == [('two', dict(bam='x.bam', fastq=None, infer_rg=False, use_oq=True, set_oq=True, gatkreport=None, output=None))]
    assert capsys.readouterr().err == ''


@pytest.mark.parametrize('argv,said', [
    (['-f', 'a.fq', 'b.fq', '--kmers'], '--kmers: only with -b/--bam'),
    (['-c', 'x.fq', '--kmers'], '--kmers: only with -b/--bam'),
    (['-b', 'x.bam', '--kmers', '--fix-n'], '--fix-n: not with -b --kmers'),
    (['-b', 'x.bam', '--kmers', '--infer-rg'], '--infer-rg: not with -b --kmers'),
    (['-b', 'x.bam', '--kmers', '--passes', '9'], 'must be in 1..8'),
    (['-b', 'x.bam', '--kmers', '--partitions', '65'], 'must be in 1..64'),
    (['-b', 'x.bam', '--filter-bits', '4'], '--filter-bits: only with -c/--correct'),
    (['-b', 'x.bam', '-k', '21'], '-k/--kmer: only with -c/--correct'),
    (['-b', 'x.bam', '--min-count', '3', '--slots', '64', '--prefilter', '--passes', '2', '--skip-unresolved', '--partitions', '2'],
     '--min-count, --slots, --prefilter, --passes, --skip-unresolved, --partitions: only with -c/--correct'),
    (['--kmers'], 'one of the arguments -b/--bam -f/--fastq -c/--correct is required'),
])
def test_argparse_errors(cli, argv, said, capsys):
    main, calls, _ = cli
    with pytest.raises(SystemExit) as e:
        main.main(['recalibrate'] + argv)
    assert e.value.code == 2 and not calls
    assert said in capsys.readouterr().err


@pytest.mark.parametrize('argv,more,line', [
    ([], {}, ''),
    (['--skip-unresolved'], dict(skipped_bases=5), ' skipped_bases=5'),
    (['--passes', '2'], dict(passes=2), ' passes=2'),
    (['--passes', '1'], {}, ''),
    (['--partitions', '3'], dict(partitions=3, kept_pairs=9, solid_slots=64), ' partitions=3'),
    (['--partitions', '3'], {}, ''),                                   # `auto` or a count that resolved to one round
    (['--prefilter'], dict(prefilter=True, admitted=99), ' prefilter=1 admitted=99 slots=2048'),
    (['--skip-unresolved', '--passes', '3', '--partitions', 'auto', '--prefilter'],
     dict(skipped_bases=5, passes=3, partitions=4, kept_pairs=9, solid_slots=64, prefilter=True, admitted=99),
     ' skipped_bases=5 passes=3 partitions=4 prefilter=1 admitted=99 slots=2048'),
])
def test_the_stderr_line_is_bqsr_kmers_own_under_another_prefix(cli, monkeypatch, capsys, argv, more, line):
    """Every optional part, in `bqsr --kmers`'s order; the same stubbed info through `bqsr` gives the same line but for the prefix."""
    from kbbq import aln
    from kbbq.gatk import bqsr
    main, calls, info = cli
    info.update(more)
    main.main(['recalibrate', '-b', 'x.sam', '--kmers', '-k', '15'] + argv)
    mine = capsys.readouterr().err
    assert mine == 'kbbq recalibrate: k=15 min_count=4 reads=600 flagged_bases=77%s\n' % line

    class Report:
        def write(self, path):
            pass
    monkeypatch.setattr(aln, 'AlignmentFile', lambda path: path)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', lambda bam, info, **kw: info.update(cli[2]) or Report())
    main.main(['bqsr', '-b', 'x.sam', '--kmers', '-k', '15', '-g', 'm.grp'] + argv)
    theirs = capsys.readouterr().err
    assert theirs.startswith('kbbq bqsr:') and 'kbbq recalibrate:' + theirs[len('kbbq bqsr:'):] == mine


def test_the_dispatcher_keeps_its_not_implemented_cases():
    from kbbq import recalibrate
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate_bam(None)
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate_bam('foo', True, True)
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate(fastq=None, bam='foo')
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate(fastq=None, bam='foo', gatkreport='foo')
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate(fastq=None, bam=None, gatkreport='foo')
    with pytest.raises(ValueError, match='only with a BAM'):
        recalibrate.recalibrate(fastq=['a.fq', 'b.fq'], bam=None, kmers={})
    with pytest.raises(TypeError, match='unknown k-mer option fix_n'):
        recalibrate.recalibrate_bam('foo', kmers=dict(fix_n=True))


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device and the collectives fails the test; reading the alignments (the host reader) does not."""
    from kbbq import _device, kmer, parallel, recalibrate
    from kbbq.gatk import applybqsr, bqsr

    def boom(*a, **kw):
        raise AssertionError('a device call or a collective was made')
    for mod, names in ((kmer, ('_ctx', 'prefilter_kmers', 'count_kmers', 'flag_errors', 'KmerTable', 'KmerFilter', 'count_partitioned',
                               'count_block', 'count_rounds')),
                       (_device, ('context', 'warm_up', 'device_budget', 'use_native_memory', '_torch')),
                       (bqsr, ('_kmer_tally', '_tally_flag_plane')),
                       (applybqsr, ('_resident_slabs', '_recalibrated_slabs', 'write_alignments')),
                       (parallel, ('all_gather_object', 'broadcast_object', 'raise_first_error', 'barrier',
                                   'allreduce_tables', 'in_rank_order', 'sum_over_ranks', 'max_over_ranks'))):
        for name in names:
            monkeypatch.setattr(mod, name, boom)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    return recalibrate


def _both(recalibrate, exc, match, path, argv, **kw):
    """The API and the command line refuse alike; the message names this command."""
    from kbbq import main
    kmers = kw.pop('kmers', {})
    with pytest.raises(exc, match=match) as e:
        recalibrate.recalibrate_bam(path, kmers=kmers, **kw)
    with pytest.raises(exc, match=match):
        main.main(['recalibrate', '-b', path, '--kmers'] + argv)
    assert 'recalibrate -b --kmers' in str(e.value) and 'bqsr --kmers' not in str(e.value).replace('`kbbq bqsr -b aln.bam --kmers', '')
    return str(e.value)


def test_check_bam_kmers_reads_nothing(no_device, tmp_path, monkeypatch):
    """The options' refusals come before the file is opened: the path does not exist."""
    from kbbq import _native
    monkeypatch.setattr(_native, 'load', lambda: (_ for _ in ()).throw(AssertionError('the library was loaded')))
    absent = str(tmp_path / 'absent.sam')
    _both(no_device, ValueError, 'k must be in 8..32, got 7', absent, ['-k', '7'], kmers=dict(k=7))
    _both(no_device, ValueError, 'k must be in 8..32, got 33', absent, ['-k', '33'], kmers=dict(k=33))
    _both(no_device, ValueError, 'min_count must be >= 1, got 0', absent, ['--min-count', '0'], kmers=dict(min_count=0))
    _both(no_device, ValueError, 'min_count must be >= 2 with the prefilter, got 1', absent, ['--prefilter', '--min-count', '1'],
          kmers=dict(prefilter=True, min_count=1))
    _both(no_device, ValueError, 'filter_bits must be in 1..64, got 65', absent, ['--prefilter', '--filter-bits', '65'],
          kmers=dict(prefilter=True, filter_bits=65))
    _both(no_device, ValueError, r'writes SAM text; BAM output \(.*x\.BAM\) is not supported', absent, ['-o', str(tmp_path / 'x.BAM')],
          output=str(tmp_path / 'x.BAM'))
    grp = tmp_path / 'model.grp'
    grp.write_text('#:GATKReport.v1.1:5\n')
    msg = _both(no_device, ValueError, 'model.grp exists', absent, ['-g', str(grp)], gatkreport=str(grp))
    assert 'kbbq applybqsr' in msg and grp.read_text() == '#:GATKReport.v1.1:5\n'
    with pytest.raises(ValueError, match='passes must be an integer in 1..8'):
        no_device.recalibrate_bam(absent, kmers=dict(passes=9))
    with pytest.raises(ValueError, match='partitions'):
        no_device.recalibrate_bam(absent, kmers=dict(partitions=65))
    assert not (tmp_path / 'x.BAM').exists()


@pytest.mark.parametrize('how', ['group', 'launcher'])
@pytest.mark.parametrize('world,rank', [(1, 0), (2, 0), (2, 1)])
def test_a_rank_refuses_with_no_collective_started(no_device, tmp_path, monkeypatch, how, world, rank):
    from kbbq import kmer, parallel
    monkeypatch.setattr(parallel, 'init_from_env', lambda: pytest.fail('the process group was joined'))
    if how == 'group':
        monkeypatch.setattr(kmer, '_ranks', lambda: (world, rank))
    else:
        monkeypatch.setenv('RANK', str(rank))
        monkeypatch.setenv('WORLD_SIZE', str(world))
        monkeypatch.setenv('KBBQ_DIST_ALWAYS', '1')
    out = tmp_path / 'out.sam'
    # the group's refusal comes first: before the options', whose messages would differ from rank to rank only by accident
    msg = _both(no_device, ValueError, 'does not run across ranks', str(tmp_path / 'absent.sam'), ['-o', str(out), '-k', '7', '--partitions', '2'],
                output=str(out), kmers=dict(k=7, partitions=2))
    assert 'kbbq bqsr -b aln.bam --kmers' in msg and 'on one GPU' in msg and 'kbbq applybqsr' in msg and 'under ranks' in msg
    assert not out.exists()


def test_the_records_refusals_come_before_any_device_work(no_device, tmp_path):
    good = [_record(i, oq='F' * 20) for i in range(4)]
    out = str(tmp_path / 'out.sam')
    p = _sam(tmp_path, good[:2] + [_record(2, seq='ACGTACGTACGTACGTACGTAC')] + good[3:], 'lengths.sam')
    msg = _both(no_device, ValueError, r'record 2 \(r2\) has 22 bases but record 0 has 20', p, ['-o', out], output=out)
    assert 'recalibrate -b --kmers needs records of one query length' in msg
    p = _sam(tmp_path, good[:1] + [_record(1, rg=None)] + good[2:], 'norg.sam')
    _both(no_device, KeyError, "tag 'RG' not present", p, ['-o', out], output=out)
    p = _sam(tmp_path, good[:3] + [_record(3, qual='*')], 'star.sam')
    msg = _both(no_device, ValueError, r"record 3 \(r3\) has QUAL '\*'", p, ['-o', out], output=out)
    assert 'recalibrate -b --kmers needs a quality for every base' in msg
    p = _sam(tmp_path, good[:3] + [_record(3)], 'nooq.sam')
    _both(no_device, KeyError, r"tag 'OQ' not present in record 3 \(r3\)", p, ['-u', '-o', out], use_oq=True, output=out)
    assert not os.path.exists(out)


def test_bam_to_kmer_covariates_keeps_its_own_refusals(no_device, tmp_path, monkeypatch):
    from kbbq import aln, kmer
    from kbbq.gatk import bqsr
    good = [_record(i) for i in range(3)]
    bam = aln.AlignmentFile(_sam(tmp_path, good + [_record(3, seq='ACGTACGTACGTACGTACGTAC')]))
    with pytest.raises(ValueError, match='so bqsr --kmers needs records of one query length'):
        bqsr.bam_to_kmer_covariates(bam, k=15)
    monkeypatch.setattr(kmer, '_ranks', lambda: (2, 1))
    with pytest.raises(ValueError, match='bqsr --kmers does not run across ranks yet'):
        bqsr.bam_to_kmer_covariates(bam, k=15)


def test_a_report_parsed_from_its_text_is_the_report_parsed_from_its_file():
    """What recalibrate_bam does in the place of writing the report and reading it back: the same parser on the same bytes, so
    EstimatedQReported comes back with the four decimals the text has."""
    from kbbq import recaltable
    from kbbq.gatk import applybqsr
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'report_short_64_1rg.txt')
    with open(path) as fh:
        text = fh.read()
    a = recaltable.RecalibrationReport.fromfile(path)
    b = recaltable.RecalibrationReport.fromtext(text)
    assert a == b and str(a) == str(b) == text
    rgs = list(a.tables[2].data.index)
    assert rgs
    for x, y in zip(applybqsr.table_to_vectors(a, rgs), applybqsr.table_to_vectors(b, rgs)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    meanq = applybqsr.table_to_vectors(b, rgs)[0]
    assert meanq.dtype == np.float64 and np.array_equal(meanq, np.round(meanq, 4))
    with pytest.raises(ValueError, match='announces 5 tables, 0 found'):
        recaltable.RecalibrationReport.fromtext('#:GATKReport.v1.1:5\n')
