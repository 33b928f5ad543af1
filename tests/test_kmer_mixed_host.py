"""`--mixed-lengths` and `-F / --exclude-flags` of `kbbq bqsr --kmers` and `kbbq recalibrate -b --kmers`, host side, no GPU: the
command lines forward the two options and refuse them where they do not belong, what the commands refuse of the records they still
refuse before any device call or collective, a record that -F leaves out is exempt from exactly three of those refusals, the
one-length refusal is what it was without --mixed-lengths, and the CPU model (tests/kmer_mixed_model.py) is kmer_bqsr_model on a
file of one length."""
import numpy as np
import pytest

import kmer_bqsr_model as B
import kmer_mixed_model as MX

HEADER = ['@HD\tVN:1.6\tSO:unsorted', '@SQ\tSN:chr1\tLN:1000', '@RG\tID:g0\tPU:unit0\tSM:s', '@RG\tID:g1\tPU:unit1\tSM:s']
SEQ = 'ACGTACGTACGTACGTACGT'


def _record(i, seq=SEQ, qual=None, rg='g0', oq=None, flag=0, cigar=None):
    qual = 'I' * len(seq) if qual is None else qual
    tags = ([] if rg is None else ['RG:Z:%s' % rg]) + ([] if oq is None else ['OQ:Z:%s' % oq])
    cigar = ('%dM' % len(seq) if seq != '*' else '*') if cigar is None else cigar
    return '\t'.join(['r%d' % i, str(flag), 'chr1', str(10 + i), '60', cigar, '*', '0', '0', seq, qual] + tags)


def _sam(tmp_path, records, name='aln.sam'):
    p = tmp_path / name
    p.write_text('\n'.join(HEADER + records) + '\n')
    return str(p)


# ---------------------------------------------------------------- command lines
class _Report:
    def write(self, path):
        pass


@pytest.fixture
def cli(monkeypatch):
    """main.main with `bqsr --kmers` and every recalibrate path recorded instead of run."""
    from kbbq import aln, main, recalibrate
    from kbbq.gatk import bqsr
    calls = []
    info = dict(k=15, min_count=4, reads=600, flagged_bases=77, slots=2048, prefilter=False, admitted=None, excluded_reads=9)
    monkeypatch.setattr(aln, 'AlignmentFile', lambda path: path)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', lambda bam, info, **kw: calls.append(('bqsr', kw)) or info.update(cli_info) or _Report())
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: calls.append(('report', a)) or _Report())
    monkeypatch.setattr(recalibrate, 'check_bam_records', lambda *a, **kw: calls.append(('records', a, kw)))
    monkeypatch.setattr(recalibrate, 'check_bam_kmers', lambda *a, **kw: calls.append(('check', a, kw)))
    monkeypatch.setattr(recalibrate, 'recalibrate', lambda **kw: calls.append(('two', kw)))
    monkeypatch.setattr(recalibrate, 'recalibrate_corrected', lambda path, **kw: calls.append(('one', kw)))
    monkeypatch.setattr(recalibrate, 'recalibrate_bam', lambda bam, **kw: calls.append(('bam', kw)) or dict(info))
    cli_info = info
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                # the command then leaves the memory back end alone
    return main, calls


def test_bqsr_forwards_the_two_options(cli, capsys):
    main, calls = cli
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-k', '15', '--mixed-lengths', '-F', '0xF00', '-g', 'r.grp'])
    assert calls == [('bqsr', dict(k=15, min_count=None, slots=None, prefilter=False, filter_bits=4, use_oq=False, mixed_lengths=True,
                                   exclude_flags=0xF00))]
    assert capsys.readouterr().err == 'kbbq bqsr: k=15 min_count=4 reads=600 excluded_reads=9 flagged_bases=77\n'
    del calls[:]
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-k', '15', '--exclude-flags', '1024', '-g', 'r.grp'])
    assert calls[0][1]['exclude_flags'] == 1024 and 'mixed_lengths' not in calls[0][1]
    del calls[:]
    # -F 0 is the command without the option: the call and the line are what they were
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-k', '15', '-F', '0', '-g', 'r.grp'])
    assert calls == [('bqsr', dict(k=15, min_count=None, slots=None, prefilter=False, filter_bits=4, use_oq=False))]
    assert capsys.readouterr().err.endswith('kbbq bqsr: k=15 min_count=4 reads=600 flagged_bases=77\n')


def test_recalibrate_forwards_the_two_options(cli, capsys):
    main, calls = cli
    main.main(['recalibrate', '-b', 'x.sam', '--kmers', '--mixed-lengths', '-F', '0xc00', '-u'])
    assert calls[0] == ('check', ('x.sam', None, None, 31, None, False, 4), dict(exclude_flags=0xC00))
    assert calls[1] == ('records', ('x.sam', True, 31, None, False, 4), dict(mixed_lengths=True, exclude_flags=0xC00))
    assert calls[2] == ('bam', dict(use_oq=True, set_oq=False, gatkreport=None, output=None,
                                    kmers=dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, mixed_lengths=True,
                                               exclude_flags=0xC00)))
    assert capsys.readouterr().err == 'kbbq recalibrate: k=15 min_count=4 reads=600 excluded_reads=9 flagged_bases=77\n'
    del calls[:]
    main.main(['recalibrate', '-b', 'x.sam', '--kmers', '--mixed-lengths'])
    assert calls[0] == ('check', ('x.sam', None, None, 31, None, False, 4), {})
    assert calls[1] == ('records', ('x.sam', False, 31, None, False, 4), dict(mixed_lengths=True))
    assert calls[2][1]['kmers'] == dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, mixed_lengths=True)
    assert capsys.readouterr().err == 'kbbq recalibrate: k=15 min_count=4 reads=600 flagged_bases=77\n'


@pytest.mark.parametrize('argv,said', [
    (['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--mixed-lengths'], '--mixed-lengths: only with --kmers'),
    (['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '-F', '0xF00'], '-F/--exclude-flags: only with --kmers'),
    (['bqsr', '-b', 'x', '-g', 'r', '--mixed-lengths', '--exclude-flags', '4'], '--mixed-lengths, -F/--exclude-flags: only with --kmers'),
    (['recalibrate', '-b', 'x.bam', '--mixed-lengths'], '--mixed-lengths: only with -b --kmers'),
    (['recalibrate', '-b', 'x.bam', '-F', '0x400'], '-F/--exclude-flags: only with -b --kmers'),
    (['recalibrate', '-c', 'x.fq', '--mixed-lengths'], '--mixed-lengths: only with -b --kmers'),
    (['recalibrate', '-f', 'a.fq', 'b.fq', '-F', '4'], '-F/--exclude-flags: only with -b --kmers'),
    (['recalibrate', '-f', 'a.fq', 'b.fq', '--kmers', '--mixed-lengths'], '--mixed-lengths: only with -b --kmers'),
    (['bqsr', '-b', 'x', '--kmers', '-g', 'r', '-F', '0x'], 'is not an integer'),
    (['bqsr', '-b', 'x', '--kmers', '-g', 'r', '-F', 'dup'], 'is not an integer'),
    (['bqsr', '-b', 'x', '--kmers', '-g', 'r', '-F', '1.5'], 'is not an integer'),
    (['bqsr', '-b', 'x', '--kmers', '-g', 'r', '-F', '0b11'], 'is not an integer'),
    (['bqsr', '-b', 'x', '--kmers', '-g', 'r', '-F', '65536'], 'must be in 0..0xFFFF'),
    (['bqsr', '-b', 'x', '--kmers', '-g', 'r', '-F', '0x10000'], 'must be in 0..0xFFFF'),
    (['recalibrate', '-b', 'x', '--kmers', '--exclude-flags=-1'], 'must be in 0..0xFFFF'),
    (['recalibrate', '-b', 'x', '--kmers', '-F', 'F00'], 'is not an integer'),
])
def test_argparse_errors(cli, argv, said, capsys):
    main, calls = cli
    with pytest.raises(SystemExit) as e:
        main.main(argv)
    assert e.value.code == 2 and not calls
    assert said in capsys.readouterr().err


def test_the_help_texts_name_the_baserecalibrator_set(capsys):
    from kbbq import main
    for command in ('bqsr', 'recalibrate'):
        with pytest.raises(SystemExit):
            main.main([command, '--help'])
        text = ' '.join(capsys.readouterr().out.split())
        assert '-F 0xF00' in text and 'secondary, QC-fail, duplicate and supplementary' in text and '--mixed-lengths' in text


# ---------------------------------------------------------------- refusals before any device call
@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device and the collectives fails the test; reading the alignments (the host reader) does not."""
    from kbbq import _device, kmer, parallel, recalibrate
    from kbbq.gatk import applybqsr, bqsr

    def boom(*a, **kw):
        raise AssertionError('a device call or a collective was made')
    for mod, names in ((kmer, ('_ctx', 'prefilter_kmers', 'count_kmers', 'flag_errors', 'kmer_histogram', 'KmerTable', 'KmerFilter',
                               'count_partitioned', 'count_block', 'count_rounds')),
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


def _all(recalibrate, exc, match, path, argv=(), use_oq=False, **kmers):
    """The two library calls and the two command lines refuse alike, with the options on."""
    from kbbq import aln, main
    from kbbq.gatk import bqsr
    kmers = dict(dict(mixed_lengths=True), **kmers)
    with pytest.raises(exc, match=match):
        bqsr.bam_to_kmer_covariates(aln.AlignmentFile(path), use_oq=use_oq, **dict(dict(k=15), **kmers))
    with pytest.raises(exc, match=match):
        recalibrate.recalibrate_bam(path, use_oq=use_oq, kmers=dict(dict(k=15), **kmers))
    flags = ['--mixed-lengths'] + (['-F', hex(kmers['exclude_flags'])] if 'exclude_flags' in kmers else []) + (['-u'] if use_oq else [])
    with pytest.raises(exc, match=match):
        main.main(['bqsr', '-b', path, '--kmers', '-g', path + '.grp'] + (['-k', '15'] if '-k' not in argv else []) + flags + list(argv))
    with pytest.raises(exc, match=match):
        main.main(['recalibrate', '-b', path, '--kmers'] + (['-k', '15'] if '-k' not in argv else []) + flags + list(argv))


def test_the_refusals_that_stay(no_device, tmp_path, monkeypatch):
    from kbbq import parallel
    monkeypatch.setattr(parallel, 'init_from_env', lambda: (1, 0))
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')
    good = [_record(i, oq='F' * 20) for i in range(4)]
    shorter = _record(2, seq=SEQ[:17], oq='F' * 17)
    ok = good[:2] + [shorter] + good[3:]
    p = _sam(tmp_path, good[:2] + [_record(2, seq=SEQ[:17], qual='I' * 16, oq='F' * 17)] + good[3:], 'count.sam')
    _all(no_device, ValueError, r'record 2 \(r2\) has 16 qualities for 17 bases', p)
    p = _sam(tmp_path, good[:2] + [_record(2, seq=SEQ[:17], qual='I' * 17, oq='F' * 18)] + good[3:], 'oqcount.sam')
    _all(no_device, ValueError, r'record 2 \(r2\) has 18 qualities for 17 bases', p, use_oq=True)
    p = _sam(tmp_path, ok[:3] + [_record(3, qual='*', oq='F' * 20)], 'star.sam')
    _all(no_device, ValueError, r"record 3 \(r3\) has QUAL '\*'", p)
    p = _sam(tmp_path, ok[:3] + [_record(3)], 'nooq.sam')
    _all(no_device, KeyError, r"tag 'OQ' not present in record 3 \(r3\)", p, use_oq=True)
    p = _sam(tmp_path, ok[:1] + [_record(1, rg=None)] + ok[2:], 'norg.sam')
    _all(no_device, KeyError, "tag 'RG' not present", p)
    p = _sam(tmp_path, ok[:3] + [_record(3, seq='*', qual='*', oq='')], 'empty.sam')
    _all(no_device, ValueError, r"record 3 \(r3\) has QUAL '\*'", p)
    _all(no_device, ValueError, r'record 3 \(r3\) has no bases', p, use_oq=True)
    p = _sam(tmp_path, ok, 'ok.sam')
    _all(no_device, ValueError, 'k must be in 8..32, got 7', p, ['-k', '7'], k=7)
    _all(no_device, ValueError, 'k must be in 8..32, got 33', p, ['-k', '33'], k=33)
    _all(no_device, ValueError, 'min_count must be >= 2 with the prefilter, got 1', p, ['--prefilter', '--min-count', '1'],
         prefilter=True, min_count=1)
    out = str(tmp_path / 'x.bam')
    with pytest.raises(ValueError, match='BAM output'):
        no_device.recalibrate_bam(p, output=out, kmers=dict(k=15, mixed_lengths=True, exclude_flags=0x400))
    from kbbq import main
    with pytest.raises(ValueError, match='BAM output'):
        main.main(['recalibrate', '-b', p, '--kmers', '--mixed-lengths', '-F', '0x400', '-o', out])


def test_the_library_refuses_a_bad_exclude_flags_word(no_device, tmp_path):
    from kbbq import aln
    from kbbq.gatk import bqsr
    p = _sam(tmp_path, [_record(i) for i in range(3)])
    for bad in (-1, 0x10000, '0x400', 1.5, True):
        with pytest.raises(ValueError, match='exclude_flags must be an integer in 0..0xFFFF'):
            bqsr.bam_to_kmer_covariates(aln.AlignmentFile(p), k=15, exclude_flags=bad)
        with pytest.raises(ValueError, match='exclude_flags must be an integer in 0..0xFFFF'):
            no_device.recalibrate_bam(str(tmp_path / 'absent.sam'), kmers=dict(k=15, exclude_flags=bad))


@pytest.mark.parametrize('how', ['group', 'launcher'])
def test_a_rank_refuses_with_the_options_on(no_device, tmp_path, monkeypatch, how):
    from kbbq import aln, kmer, main, parallel
    from kbbq.gatk import bqsr
    p = _sam(tmp_path, [_record(0), _record(1, seq=SEQ[:17])])
    bam = aln.AlignmentFile(p)
    monkeypatch.setattr(parallel, 'init_from_env', lambda: pytest.fail('the process group was joined'))
    if how == 'group':
        monkeypatch.setattr(kmer, '_ranks', lambda: (2, 1))
        with pytest.raises(ValueError, match='bqsr --kmers does not run across ranks yet'):
            bqsr.bam_to_kmer_covariates(bam, k=15, mixed_lengths=True, exclude_flags=0x400)
    else:
        monkeypatch.setenv('RANK', '1')
        monkeypatch.setenv('WORLD_SIZE', '2')
        monkeypatch.setenv('KBBQ_DIST_ALWAYS', '1')
    with pytest.raises(ValueError, match='recalibrate -b --kmers does not run across ranks yet'):
        no_device.recalibrate_bam(p, kmers=dict(k=15, mixed_lengths=True, exclude_flags=0x400))
    with pytest.raises(ValueError, match='recalibrate -b --kmers does not run across ranks yet'):
        main.main(['recalibrate', '-b', p, '--kmers', '--mixed-lengths', '-F', '0x400'])


def test_an_excluded_record_is_exempt_from_three_refusals_and_no_other(no_device, tmp_path):
    from kbbq import aln
    from kbbq.gatk import bqsr
    good = [_record(i, oq='F' * 20) for i in range(3)]
    run = lambda path, use_oq=False, **kw: bqsr._kmer_inputs(aln.AlignmentFile(path), 15, None, False, 4, use_oq, 42, **kw)
    # QUAL '*', no OQ tag, no SEQ: refused of a record that counts, passed over of one that does not
    for name, odd, use_oq, said in (('star', _record(3, qual='*', oq='F' * 20, flag=0x800), False, "has QUAL"),
                                    ('nooq', _record(3, flag=0x800), True, "tag 'OQ' not present"),
                                    ('empty', _record(3, seq='*', qual='*', flag=0x800), False, "has QUAL"),
                                    ('empty_u', _record(3, seq='*', qual='*', flag=0x800), True, "tag 'OQ' not present")):
        p = _sam(tmp_path, good + [odd], name + '.sam')
        with pytest.raises((ValueError, KeyError), match=said):
            run(p, use_oq, mixed_lengths=True)
        with pytest.raises((ValueError, KeyError), match=said):
            run(p, use_oq, mixed_lengths=True, exclude_flags=0x400)          # another bit: the record counts
        b, n, S, excluded = run(p, use_oq, mixed_lengths=True, exclude_flags=0x800)
        assert (n, S) == (4, 20) and excluded.tolist() == [False, False, False, True]
    # a record of no bases that counts
    p = _sam(tmp_path, good + [_record(3, seq='*', qual='*', oq='', flag=0x800)], 'nobases.sam')
    with pytest.raises(ValueError, match=r'record 3 \(r3\) has no bases'):
        run(p, True, mixed_lengths=True)
    assert run(p, True, mixed_lengths=True, exclude_flags=0x800)[3].tolist() == [False, False, False, True]
    # not exempt: RG, and qualities that are there in another number than the bases
    p = _sam(tmp_path, good + [_record(3, rg=None, flag=0x800)], 'norg.sam')
    with pytest.raises(KeyError, match="tag 'RG' not present"):
        run(p, mixed_lengths=True, exclude_flags=0x800)
    p = _sam(tmp_path, good + [_record(3, qual='I' * 19, flag=0x800)], 'count.sam')
    with pytest.raises(ValueError, match=r'record 3 \(r3\) has 19 qualities for 20 bases'):
        run(p, mixed_lengths=True, exclude_flags=0x800)
    # S is the longest record, excluded ones included; without the option the tuple is the one it was
    p = _sam(tmp_path, good + [_record(3, seq=SEQ + 'ACGT', flag=0x400)], 'longest.sam')
    b, n, S, excluded = run(p, mixed_lengths=True, exclude_flags=0xC00)
    assert S == 24 and int(excluded.sum()) == 1
    assert len(run(p, mixed_lengths=True)) == 3 and run(p, mixed_lengths=True)[2] == 24


def test_without_mixed_lengths_the_refusal_is_what_it_was(no_device, tmp_path, monkeypatch):
    from kbbq import aln, main, parallel
    from kbbq.gatk import bqsr
    monkeypatch.setattr(parallel, 'init_from_env', lambda: (1, 0))
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')
    p = _sam(tmp_path, [_record(0), _record(1), _record(2, seq=SEQ + 'AC'), _record(3)])
    old = (r'^record 2 \(r2\) has 22 bases but record 0 has 20: the tally has one cycle axis of 2 S, so %s needs records of one query '
           r'length')
    for kw in ({}, dict(exclude_flags=0x800), dict(mixed_lengths=False)):
        with pytest.raises(ValueError, match=old % 'bqsr --kmers') as e:
            bqsr.bam_to_kmer_covariates(aln.AlignmentFile(p), k=15, **kw)
        assert '--mixed-lengths' in str(e.value)                           # the hint behind the message
        with pytest.raises(ValueError, match=old % 'recalibrate -b --kmers'):
            no_device.recalibrate_bam(p, kmers=dict(k=15, **kw))
    with pytest.raises(ValueError, match=old % 'bqsr --kmers'):
        main.main(['bqsr', '-b', p, '--kmers', '-k', '15', '-g', str(tmp_path / 'r.grp')])
    with pytest.raises(ValueError, match=old % 'recalibrate -b --kmers'):
        main.main(['recalibrate', '-b', p, '--kmers', '-k', '15', '-F', '0x800'])
    # with it the records pass: (batch, n, S) with S the longest
    b, n, S = no_device.check_bam_records(aln.AlignmentFile(p), k=15, mixed_lengths=True)
    assert (n, S) == (4, 22) and b.qlen.tolist() == [20, 20, 22, 20]
    with pytest.raises(TypeError, match='unknown k-mer option mixed'):
        no_device.recalibrate_bam(p, kmers=dict(mixed=True))


# ---------------------------------------------------------------- the model and its fixtures
@pytest.fixture(scope='module')
def synth(tmp_path_factory):
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('kmer_mixed_host')
    paths = OQ.synth_bqsr_set(str(d), **B.FIXTURE)
    return dict(dir=d, paths=paths, text=open(paths['sam']).read())


def test_on_one_length_the_model_is_kmer_bqsr_model(synth):
    reads, rgs, _ = B.load(synth['paths']['sam'])
    for use_oq in (False, True):
        want, winfo = B.vectors(reads, rgs, 15, use_oq=use_oq)
        got, info = MX.vectors(reads, rgs, 15, use_oq=use_oq)
        for name, g, w in zip(B.VEC, got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True), name
        assert {k: info[k] for k in winfo} == winfo and info['excluded_reads'] == 0 and info['skipped_bases'] == 0
    B.check_share(winfo)


def test_the_fixtures_are_what_a_trimmer_leaves(synth):
    """SEQ, QUAL, OQ and CIGAR cut alike; the product's reader and the oracle's stand-ins see the same records; an excluded record
    is out of the model's flags and its tally."""
    from kbbq import aln
    p = synth['dir'] / 'mixed.sam'
    p.write_text(MX.shorten(synth['text'], 'mixed'))
    reads, rgs, _ = MX.load(str(p))
    whole = B.load(synth['paths']['sam'])[0]
    b = aln.AlignmentFile(str(p)).batch()
    lens = np.array([len(r.query_sequence) for r in reads])
    assert np.array_equal(b.qlen, lens) and np.array_equal(b.qual_len, lens) and np.array_equal(b.oq_len, lens)
    assert np.array_equal(b.clip, np.array([r.query_alignment_start | (r.query_alignment_end << 16) for r in reads], dtype=np.uint32))
    seq = b.plane(0, 64)
    assert all(not seq[i, lens[i]:].any() for i in range(600))             # the contract of the planes: 0 at and behind the length
    at_start = at_end = 0
    for r, w in zip(reads, whole):
        L = len(r.query_sequence)
        if w.query_sequence.endswith(r.query_sequence) and L < 60:
            at_start += 1
            assert r.reference_end == w.reference_end and r.reference_start >= w.reference_start
            assert r.get_tag('OQ') == w.get_tag('OQ')[-L:]
        elif L < 60:
            at_end += 1
            assert w.query_sequence.startswith(r.query_sequence) and r.reference_start == w.reference_start
            assert r.get_tag('OQ') == w.get_tag('OQ')[:L]
        assert not any(op == 5 for op, _ in r.cigartuples) and sum(n for op, n in r.cigartuples if op in (0, 1, 4, 7, 8)) == L
    assert at_start >= 80 and at_end >= 80
    mask = np.arange(600) % 7 == 0
    err, t = MX.flags(reads, 15, exclude=mask)
    got, info = MX.vectors(reads, rgs, 15, exclude=mask, flagged=(err, t))
    kept = [r for r, m in zip(reads, mask) if not m]
    want, winfo = MX.vectors(kept, rgs, 15)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)) and not err[mask].any()
    assert info['excluded_reads'] == 86 and {k: v for k, v in info.items() if k != 'excluded_reads'} == \
        {k: v for k, v in winfo.items() if k != 'excluded_reads'}
    MX.check_share(info)
