"""`kbbq bqsr --kmers --mixed-lengths [-F INT]` and `kbbq recalibrate -b --kmers --mixed-lengths [-F INT]` on the MI355X:
kbbq.gatk.bqsr.bam_to_kmer_covariates(mixed_lengths=True, exclude_flags=..) against the CPU model (tests/kmer_mixed_model.py) on
records of several query lengths -- the fused tally, the 4-bit canonical rows and the character rows, SAM and BAM, QUAL and OQ,
prefilter, passes, skip-unresolved, partitions -- and the command lines byte for byte.

Fixtures (kmer_mixed_model.shorten over oracle_bqsr.synth_bqsr_set(**kmer_bqsr_model.FIXTURE), 600 records, 3 read groups):
  mixed  every third record cut to 60, 59, 48, 47, 33, 32, 31, 17, 16, 14 bases in turn, at the stored SEQ's end or its start
  short  every record cut to 31, 30, 24, 17, 16 bases in turn: S = 31, the fused tally declines and the canonical rows run
Share of all bases the model alone flags (kmer_bqsr_model.check_share asks for 1 %..10 %), measured on the CPU:
  mixed  k=15 at the valley (min_count 11)  586 / 31140 = 1.88 %     k=21 min_count=3  588 / 31140 = 1.89 %
  short  k=15 at the valley (min_count 8)    64 / 14160 = 0.45 %: too few, so min_count is fixed at 3: 1.60 %
  mixed with 0x800 on every 7th and 0x400 on every 11th record (133 records) left out:
         k=15 at the valley (min_count 9)   461 / 24246 = 1.90 % of the bases of the records that count
  mixed, two passes at k=15 with the unresolved bases left out: 824 / 31140 = 2.65 % flagged (11202 bases unresolved)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_mixed_model as MX

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED'):
    ENV.pop(_var, None)

_memo = {}
SHORT_MIN_COUNT = 3


def _records(text):
    return [ln.split('\t') for ln in text.split('\n') if ln and not ln.startswith('@')]


def _edit(text, fn):
    """The SAM text with fn(index, fields) -> fields, or None to delete the record, applied to every record."""
    out, idx = [], 0
    for ln in text.split('\n'):
        if ln and not ln.startswith('@'):
            f = fn(idx, ln.split('\t'))
            idx += 1
            if f is None:
                continue
            ln = '\t'.join(f)
        out.append(ln)
    return '\n'.join(out)


def _flag_bits(i):
    return (0x800 if i % 7 == 0 else 0) | (0x400 if i % 11 == 0 else 0)


@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    import bamwriter
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('bqsr_mixed')
    paths = OQ.synth_bqsr_set(str(d), **MX.FIXTURE)
    whole = open(paths['sam']).read()
    fx = dict(dir=d, paths={'whole': paths['sam']}, reads={})

    def add(name, text, bam=False):
        p = d / (name + '.sam')
        p.write_text(text)
        fx['paths'][name] = str(p)
        fx['reads'][name], fx['rgs'], fx['pus'] = MX.load(str(p))
        if bam:
            fx['paths'][name + '.bam'] = str(bamwriter.write_bam(d / (name + '.bam'), text))
        return text
    mixed = add('mixed', MX.shorten(whole, 'mixed'), bam=True)
    add('short', MX.shorten(whole, 'short'))
    marked = add('marked', _edit(mixed, lambda i, f: f[:1] + [str(int(f[1]) | _flag_bits(i))] + f[2:]), bam=True)
    add('deleted', _edit(marked, lambda i, f: None if _flag_bits(i) else f))
    reads = fx['reads']['mixed']
    before = _records(whole)
    lens = [len(r.query_sequence) for r in reads]
    assert len(reads) == 600 and len(fx['rgs']) == 3 and max(lens) == 60
    assert sorted(set(lens)) == sorted(MX.MIXED_LENGTHS) and sum(1 for x, f in zip(lens, before) if x != len(f[9])) == 180
    assert any(r.is_reverse and r.is_read2 and len(r.query_sequence) <= 32 for r in reads)
    assert any(not r.is_reverse and len(r.query_sequence) <= 32 for r in reads)
    assert any(OQ.trim(r).any() for r, f in zip(reads, before) if len(r.query_sequence) != len(f[9]))    # a non-zero adaptor-trim word
    assert any(op == 4 for r in reads if len(r.query_sequence) < 60 for op, _ in r.cigartuples)
    assert max(len(r.query_sequence) for r in fx['reads']['short']) == 31
    fx['mask'] = np.array([_flag_bits(i) != 0 for i in range(600)])
    assert 100 < int(fx['mask'].sum()) < 160 and any(x == 60 and not m for x, m in zip(lens, fx['mask']))
    assert len(fx['reads']['deleted']) == 600 - int(fx['mask'].sum()) and max(len(r.query_sequence) for r in fx['reads']['deleted']) == 60
    return fx


def _want(fixture, key, k, t, use_oq=False, masked=False):
    """The model's vectors, computed once and left unchanged; the flagged share is checked each time."""
    exclude = fixture['mask'] if masked else None
    memo = (key, k, t, use_oq, masked)
    if memo not in _memo:
        if (key, k, t, masked) not in _memo:                # the flags do not depend on which qualities are read
            _memo[(key, k, t, masked)] = MX.flags(fixture['reads'][key], k, t, exclude)
        vec, info = MX.vectors(fixture['reads'][key], fixture['rgs'], k, t, use_oq=use_oq, exclude=exclude,
                               flagged=_memo[(key, k, t, masked)])
        for a in vec:
            a.setflags(write=False)
        _memo[memo] = (vec, info)
    vec, info = _memo[memo]
    MX.check_share(info)
    return vec, info


def _same(got, want, what=''):
    assert len(got) == 9
    for name, g, w in zip(MX.VEC, got, want):
        assert np.array_equal(g, w), (name, what)


def _fused(monkeypatch, fused):
    if fused is None:
        monkeypatch.delenv('KBBQ_TALLY_FUSED', raising=False)
    else:
        monkeypatch.setenv('KBBQ_TALLY_FUSED', fused)


CASES = [dict(k=15, min_count=None), dict(k=21, min_count=3, use_oq=True), dict(k=15, min_count=None, prefilter=True)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join('%s=%s' % kv for kv in c.items()))
@pytest.mark.parametrize('fused', [None, '0'])
@pytest.mark.parametrize('source', ['sam', 'bam'])
def test_vectors_equal_the_model(fixture, case, fused, source, monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    _fused(monkeypatch, fused)
    want, winfo = _want(fixture, 'mixed', case['k'], case['min_count'], case.get('use_oq', False))
    info = {}
    path = fixture['paths']['mixed' if source == 'sam' else 'mixed.bam']
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(path), info=info, mixed_lengths=True, **case)
    _same(got, want, (case, fused, source))
    assert got[0].dtype == np.int64 and got[5].shape[2] == 120 and int(got[1].sum()) > 100 and int(got[2].sum()) > 15000
    assert info['k'] == case['k'] and info['min_count'] == winfo['min_count'] and info['reads'] == 600
    assert info['flagged_bases'] == winfo['flagged_bases'] and 'excluded_reads' not in info
    assert (info['admitted'] is not None) == bool(case.get('prefilter'))


def test_records_all_shorter_than_32_go_through_the_canonical_rows(fixture, monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    _fused(monkeypatch, None)
    want, winfo = _want(fixture, 'short', 15, SHORT_MIN_COUNT)
    info = {}
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['short']), k=15, min_count=SHORT_MIN_COUNT, info=info,
                                      mixed_lengths=True)
    _same(got, want)
    assert got[5].shape[2] == 62 and int(got[2].sum()) > 5000
    assert info['min_count'] == SHORT_MIN_COUNT and info['reads'] == 600 and info['flagged_bases'] == winfo['flagged_bases']


def test_a_letter_outside_acgtn_in_a_short_record_runs_the_chain_down_to_character_rows(fixture, monkeypatch):
    """One forward record of 33 bases with an 'R' in its aligned part, among qualities below 6 so that no looked-up dinucleotide holds
    it: the fused tally and the 4-bit canonical rows refuse it (tables of their own), the character rows count it."""
    from kbbq import aln
    from kbbq.gatk import bqsr
    reads = fixture['reads']['mixed']
    hit = [i for i, r in enumerate(reads) if not r.is_reverse and len(r.query_sequence) == 33
           and r.query_alignment_start <= 10 and r.query_alignment_end >= 20]
    assert hit
    hit = hit[0]

    def odd(i, f):
        if i == hit:
            f[9] = f[9][:14] + 'R' + f[9][15:]
            f[10] = f[10][:14] + '$$' + f[10][16:]                      # '$' = 3 < 6
        return f
    p = fixture['dir'] / 'weird.sam'
    p.write_text(_edit(open(fixture['paths']['mixed']).read(), odd))
    fixture['reads']['weird'] = MX.load(str(p))[0]
    assert fixture['reads']['weird'][hit].query_sequence[14] == 'R' and len(fixture['reads']['weird'][hit].query_sequence) == 33
    want, _ = _want(fixture, 'weird', 15, None)
    for fused in (None, '0'):
        _fused(monkeypatch, fused)
        _same(bqsr.bam_to_kmer_covariates(aln.AlignmentFile(str(p)), k=15, mixed_lengths=True), want, fused)


def test_on_one_length_the_option_changes_nothing(fixture, monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    _fused(monkeypatch, None)
    a, b = {}, {}
    plain = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['whole']), k=15, info=a)
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['whole']), k=15, info=b, mixed_lengths=True)
    _same(got, plain)
    assert a == b and a['reads'] == 600


def test_passes_and_skip_unresolved_compose(fixture, monkeypatch):
    """The flags of two passes, unresolved bases left out: the model fed with kmer_passes_model's class plane."""
    import kmer_passes_model as PM
    from kbbq import aln
    from kbbq.gatk import bqsr
    _fused(monkeypatch, None)
    reads = fixture['reads']['mixed']
    seq, meta, _ = MX.planes(reads)
    solid, t = PM.solid_set(seq, meta, 15)
    steps = PM.trace(seq, meta, 15, t, 2, solid_keys=solid)
    cls = steps[1][2]
    assert int((cls == 2).sum()) >= 50 and int((cls == 1).sum()) >= int((steps[0][2] == 1).sum())
    want, winfo = MX.vectors(reads, fixture['rgs'], 15, flagged=(cls, t))
    MX.check_share(winfo)
    plain, _ = _want(fixture, 'mixed', 15, None)
    assert int(want[2].sum()) < int(plain[2].sum())                     # the unresolved bases are no observations
    info = {}
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['mixed']), k=15, info=info, mixed_lengths=True,
                                      skip_unresolved=True, passes=2)
    _same(got, want)
    assert info['min_count'] == t and info['flagged_bases'] == winfo['flagged_bases'] and info['skipped_bases'] == winfo['skipped_bases']
    assert info['passes'] == 2


def test_partitions_equal_the_one_table_run(fixture, monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    _fused(monkeypatch, None)
    want, winfo = _want(fixture, 'mixed', 15, None)
    info = {}
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['mixed.bam']), k=15, info=info, mixed_lengths=True, partitions=2)
    _same(got, want)
    assert info['partitions'] == 2 and info['min_count'] == winfo['min_count'] and info['flagged_bases'] == winfo['flagged_bases']


@pytest.mark.parametrize('fused', [None, '0'])
def test_excluded_records_teach_the_model_nothing(fixture, fused, monkeypatch):
    """exclude_flags=0xC00 == the model with that mask == the product on the file with those records deleted."""
    from kbbq import aln
    from kbbq.gatk import bqsr
    _fused(monkeypatch, fused)
    want, winfo = _want(fixture, 'marked', 15, None, masked=True)
    plain, _ = _want(fixture, 'mixed', 15, None)
    assert int(want[2].sum()) < int(plain[2].sum())
    a, b = {}, {}
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['marked']), k=15, info=a, mixed_lengths=True, exclude_flags=0xC00)
    _same(got, want, fused)
    nex = int(fixture['mask'].sum())
    assert a['excluded_reads'] == nex == winfo['excluded_reads'] and a['reads'] == 600
    assert a['min_count'] == winfo['min_count'] and a['flagged_bases'] == winfo['flagged_bases']
    deleted = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['deleted']), k=15, info=b, mixed_lengths=True)
    _same(deleted, want, 'deleted')
    assert b['reads'] == 600 - nex and 'excluded_reads' not in b
    assert {k: v for k, v in a.items() if k not in ('reads', 'excluded_reads')} == {k: v for k, v in b.items() if k != 'reads'}
    # bits outside the mask exclude nothing; the word is still reported
    c = {}
    _same(bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths']['marked']), k=15, info=c, mixed_lengths=True, exclude_flags=0x200), plain)
    assert c['excluded_reads'] == 0


def test_an_excluded_record_may_lack_its_qualities(fixture, monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    _fused(monkeypatch, None)
    assert fixture['mask'][7] and len(fixture['reads']['marked'][7].query_sequence) == 60

    def star(i, f):
        return f[:10] + ['*'] + f[11:] if i == 7 else f
    p = fixture['dir'] / 'star.sam'
    p.write_text(_edit(open(fixture['paths']['marked']).read(), star))
    want, _ = _want(fixture, 'marked', 15, None, masked=True)
    _same(bqsr.bam_to_kmer_covariates(aln.AlignmentFile(str(p)), k=15, mixed_lengths=True, exclude_flags=0xC00), want)
    with pytest.raises(ValueError, match=r"record 7 \(p00003\) has QUAL '\*'"):
        bqsr.bam_to_kmer_covariates(aln.AlignmentFile(str(p)), k=15, mixed_lengths=True)


# ---------------------------------------------------------------- the command lines, each command a process of its own
def _kbbq(*argv, timeout=300):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + [str(a) for a in argv], capture_output=True, timeout=timeout, env=ENV)


def _line(r, command):
    return [ln for ln in r.stderr.decode().split('\n') if ln.startswith('kbbq %s:' % command)]


def test_bqsr_command_writes_the_models_report(fixture, tmp_path):
    from kbbq.gatk import bqsr
    want, winfo = _want(fixture, 'mixed', 15, None)
    wanted = tmp_path / 'want.grp'
    bqsr.vectors_to_report(*want, fixture['pus']).write(str(wanted))
    grp = tmp_path / 'mixed.grp'
    r = _kbbq('bqsr', '-b', fixture['paths']['mixed'], '--kmers', '-k', '15', '--mixed-lengths', '-g', grp)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == b'' and grp.read_bytes() == wanted.read_bytes()
    assert _line(r, 'bqsr') == ['kbbq bqsr: k=15 min_count=%d reads=600 flagged_bases=%d' % (winfo['min_count'], winfo['flagged_bases'])]
    # without the option the file is refused as it was, by both commands, and nothing is written
    for argv, said in ((('bqsr', '-g', tmp_path / 'no.grp'), 'so bqsr --kmers needs records of one query length'),
                       (('recalibrate', '-o', tmp_path / 'no.sam'), 'so recalibrate -b --kmers needs records of one query length')):
        r = _kbbq(argv[0], '-b', fixture['paths']['mixed'], '--kmers', '-k', '15', *argv[1:])
        assert r.returncode != 0 and r.stdout == b''
        assert 'ValueError: record 3 (p00001) has 59 bases but record 0 has 60: the tally has one cycle axis of 2 S, ' + said in r.stderr.decode()
        assert not os.path.exists(argv[2])


@pytest.mark.parametrize('source,opts,exclude', [('mixed', [], []), ('marked.bam', ['-u', '-s'], ['-F', '0xC00']), ('marked', [], ['-F', '3072'])],
                         ids=['sam', 'bam-u-s-F', 'sam-F'])
def test_recalibrate_is_bqsr_then_applybqsr(fixture, tmp_path, source, opts, exclude):
    from kbbq.gatk import bqsr
    path = fixture['paths'][source]
    use_oq = '-u' in opts
    grp, grp2 = tmp_path / 'R.grp', tmp_path / 'R2.grp'
    first = _kbbq('bqsr', '-b', path, '--kmers', '-k', '15', '--mixed-lengths', *[x for x in opts if x == '-u'], *exclude, '-g', grp)
    assert first.returncode == 0, first.stderr.decode()[-3000:]
    want, winfo = _want(fixture, 'marked' if exclude else 'mixed', 15, None, use_oq=use_oq, masked=bool(exclude))
    wanted = tmp_path / 'want.grp'
    bqsr.vectors_to_report(*want, fixture['pus']).write(str(wanted))
    assert grp.read_bytes() == wanted.read_bytes()
    second = _kbbq('applybqsr', '-b', path, '-g', grp, *opts)
    assert second.returncode == 0, second.stderr.decode()[-3000:]
    one = _kbbq('recalibrate', '-b', path, '--kmers', '-k', '15', '--mixed-lengths', *opts, *exclude, '-g', grp2)
    assert one.returncode == 0, one.stderr.decode()[-3000:]
    assert one.stdout == second.stdout and grp2.read_bytes() == grp.read_bytes()
    records = _records(one.stdout.decode())
    before = _records(open(fixture['paths']['marked' if exclude else 'mixed']).read())
    assert len(records) == 600 and [len(f[10]) for f in records] == [len(f[9]) for f in before]
    assert sum(a[10] != b[10] for a, b in zip(records, before)) > 300
    tail = 'k=15 min_count=%d reads=600%s flagged_bases=%d' % (winfo['min_count'], ' excluded_reads=%d' % int(fixture['mask'].sum()) if exclude else '',
                                                             winfo['flagged_bases'])
    assert _line(one, 'recalibrate') == ['kbbq recalibrate: ' + tail] and _line(first, 'bqsr') == ['kbbq bqsr: ' + tail]
    if exclude:
        # an excluded record is recalibrated like any other
        assert sum(a[10] != b[10] for a, b, m in zip(records, before, fixture['mask']) if m) > 50
