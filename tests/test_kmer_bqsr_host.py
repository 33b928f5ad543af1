"""`kbbq bqsr --kmers`, no GPU: the command line's new options, the new C ABI symbol and its device-free refusals, the refusals of
kbbq.gatk.bqsr.bam_to_kmer_covariates that must come before any device call or collective, and the CPU model
(tests/kmer_bqsr_model.py) against the oracle's reference-based tally where the two must agree."""
import os

import numpy as np
import pytest

import kmer_bqsr_model as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('kmer_bqsr_host')
    paths = OQ.synth_bqsr_set(str(d), **B.FIXTURE)
    reads, rgs, pus = B.load(paths['sam'])
    return dict(paths=paths, reads=reads, rgs=rgs, pus=pus, dir=d)


# ---------------------------------------------------------------- command line
class _Report:
    def __init__(self, seen):
        self.seen = seen

    def write(self, path):
        self.seen['out'] = path


def _patched(monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    seen = {}

    def kmers(bam, **kw):
        seen.update(kmers=(bam, kw))
        kw['info'].update(k=kw['k'], min_count=7, reads=5, flagged_bases=11, admitted=13, slots=1024)
        return _Report(seen)
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: 'opened:' + p)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', kmers)
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: seen.update(report=a) or _Report(seen))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the command then leaves the memory back end alone
    return seen


def test_argparse_kmers_reaches_the_k_mer_report(monkeypatch, capsys):
    from kbbq import main
    seen = _patched(monkeypatch)
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp'])
    bam, kw = seen['kmers']
    info = kw.pop('info')
    assert bam == 'opened:x.bam' and seen['out'] == 'r.grp' and isinstance(info, dict)
    assert kw == dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, use_oq=False)
    assert capsys.readouterr().err == 'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11\n'
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-k', '21', '--min-count', '3', '--slots', '4096', '--prefilter', '--filter-bits', '8',
               '-u', '-g', 'r2.grp'])
    bam, kw = seen['kmers']
    kw.pop('info')
    assert kw == dict(k=21, min_count=3, slots=4096, prefilter=True, filter_bits=8, use_oq=True) and seen['out'] == 'r2.grp'
    assert capsys.readouterr().err == 'kbbq bqsr: k=21 min_count=7 reads=5 flagged_bases=11 prefilter=1 admitted=13 slots=1024\n'
    assert 'report' not in seen


@pytest.mark.parametrize('argv', [
    ['bqsr', '-b', 'x', '--kmers', '-r', 'x.fa', '-g', 'r'],
    ['bqsr', '-b', 'x', '--kmers', '-v', 'x.vcf', '-g', 'r'],
    ['bqsr', '-b', 'x', '-g', 'r', '-k', '21'],
    ['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--min-count', '3'],
    ['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--slots', '1024'],
    ['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--prefilter'],
    ['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--filter-bits', '4'],
    ['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '-u'],
    ['bqsr', '-b', 'x', '-r', 'x.fa', '-g', 'r'],
    ['bqsr', '-b', 'x', '-v', 'x.vcf', '-g', 'r'],
    ['bqsr', '-b', 'x', '-g', 'r'],
    ['bqsr', '--kmers', '-g', 'r'],
])
def test_argparse_refuses(monkeypatch, argv, capsys):
    from kbbq import main
    seen = _patched(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(argv)
    assert exc.value.code == 2 and not seen
    err = capsys.readouterr().err
    if '--kmers' not in argv and len(argv) > 7:
        assert 'only with --kmers' in err


def test_argparse_old_form_is_unchanged(monkeypatch, capsys):
    from kbbq import benchmark, main
    seen = _patched(monkeypatch)
    monkeypatch.setattr(benchmark, 'get_var_sites', lambda p: 'sites:' + p)
    main.main(['bqsr', '-b', 'in.sam', '-r', 'x.fa', '-v', 's.vcf', '-g', 'r.grp'])
    assert seen == dict(report=('opened:in.sam', 'x.fa', 'sites:s.vcf'), out='r.grp')
    out = capsys.readouterr()
    assert out.err == '' and out.out == ''


# ---------------------------------------------------------------- the C ABI
def test_symbol_is_exported_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    assert hasattr(lib, 'kbbq_kmer_flag_dev')
    assert N.PROTOTYPES['kbbq_kmer_flag_dev'] == N.PROTOTYPES['kbbq_kmer_correct_dev']
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    assert 'int kbbq_kmer_flag_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,' in header


def test_device_free_refusals_of_the_call():
    """No context and no table exist without a device: every refusal below is decided on the arguments alone."""
    from kbbq import _native as N
    lib = N.load()
    assert lib.kbbq_kmer_flag_dev(None, None, None, None, 0, 16, 2, None, None) == N.KBBQ_E_ARG          # NULL ctx and table
    assert 'kbbq_kmer_flag_dev' in N.last_error()
    buf = np.zeros(64, dtype=np.uint8)
    fake = N.ptr(buf)                                   # never dereferenced: a NULL table is refused first
    assert lib.kbbq_kmer_flag_dev(fake, None, fake, fake, 1, 16, 2, fake, None) == N.KBBQ_E_ARG
    assert lib.kbbq_kmer_flag_dev(None, fake, fake, fake, 1, 16, 2, fake, None) == N.KBBQ_E_ARG
    assert 'NULL ctx or table' in N.last_error()
    for pitch in (17, 0, 24, -16):
        assert lib.kbbq_kmer_flag_dev(None, None, None, None, 1, pitch, 2, None, None) == N.KBBQ_E_ARG
        assert 'pitch must be a positive multiple of 16' in N.last_error()
    for mc in (0, -1):
        assert lib.kbbq_kmer_flag_dev(None, None, None, None, 1, 16, mc, None, None) == N.KBBQ_E_ARG
        assert 'min_count must be >= 1' in N.last_error()


# ---------------------------------------------------------------- refusals before any device call
def _no_device(monkeypatch):
    """kbbq.kmer._ctx, _native.load and every collective raise: a refusal that arrives anyway came first."""
    from kbbq import _native, kmer, parallel

    def boom(*a, **kw):
        raise AssertionError('a device call was made')

    def collective(*a, **kw):
        raise AssertionError('a collective was started')
    monkeypatch.setattr(kmer, '_ctx', boom)
    monkeypatch.setattr(_native, 'load', boom)
    for name in ('prefilter_kmers', 'count_kmers', 'flag_errors', 'kmer_histogram'):
        monkeypatch.setattr(kmer, name, boom)
    for name in ('all_gather_object', 'sum_over_ranks', 'max_over_ranks', 'raise_first_error', 'barrier', 'all_to_all_rows',
                 'allreduce_tables', 'broadcast_object', 'all_gather_rows'):
        monkeypatch.setattr(parallel, name, collective)


def _edited(fixture, name, fn):
    """The fixture's SAM with fn(index, fields) applied to every record, opened by the product's reader."""
    from kbbq import aln
    out, idx = [], 0
    for ln in open(fixture['paths']['sam']).read().split('\n'):
        if ln and not ln.startswith('@'):
            ln = '\t'.join(fn(idx, ln.split('\t')))
            idx += 1
        out.append(ln)
    p = fixture['dir'] / name
    p.write_text('\n'.join(out))
    return aln.AlignmentFile(str(p))


def test_ranks_are_refused_before_any_collective(fixture, monkeypatch):
    from kbbq import aln, kmer
    from kbbq.gatk import bqsr
    bam = aln.AlignmentFile(fixture['paths']['sam'])
    _no_device(monkeypatch)
    for rank in (0, 1):                                  # every rank refuses, not rank 0 alone
        monkeypatch.setattr(kmer, '_ranks', lambda rank=rank: (2, rank))
        for fn in (bqsr.bam_to_kmer_covariates, bqsr.bam_to_report_kmers):
            with pytest.raises(ValueError, match=r'bqsr -r -v.*under ranks.*--kmers.*on one GPU'):
                fn(bam, k=15)
            with pytest.raises(ValueError, match='ranks'):
                fn(bam, k=15, prefilter=True)


def test_input_refusals_come_before_any_device_call(fixture, monkeypatch):
    from kbbq import kmer
    from kbbq.gatk import bqsr

    def shorter(i, f):
        if i == 7:
            f[9], f[10], f[-1], f[5] = f[9][:50], f[10][:50], f[-1][:5 + 50], '50M'
        return f

    def star(i, f):
        if i == 5:
            f[10] = '*'
        return f

    def no_oq(i, f):
        return f[:-1] if i == 9 else f

    def no_rg(i, f):
        return f[:11] + f[12:] if i == 3 else f
    mixed, starred, oqless, rgless = (_edited(fixture, n + '.sam', fn) for n, fn in
                                      (('mixed', shorter), ('star', star), ('no_oq', no_oq), ('no_rg', no_rg)))
    from kbbq import aln
    whole = aln.AlignmentFile(fixture['paths']['sam'])
    _no_device(monkeypatch)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    run = bqsr.bam_to_kmer_covariates
    with pytest.raises(ValueError, match=r'record 7 \(p00003\) has 50 bases but record 0 has 60'):
        run(mixed, k=15)
    with pytest.raises(ValueError, match=r"record 5 \(p00002\) has QUAL '\*'"):
        run(starred, k=15)
    with pytest.raises(KeyError, match='OQ'):
        run(oqless, k=15, use_oq=True)
    with pytest.raises(KeyError, match='RG'):
        run(rgless, k=15)
    for mc in (1, 0):
        with pytest.raises(ValueError, match='min_count'):
            run(whole, k=15, prefilter=True, min_count=mc)
    with pytest.raises(ValueError, match='min_count'):
        run(whole, k=15, min_count=0)
    with pytest.raises(ValueError, match='filter_bits'):
        run(whole, k=15, prefilter=True, filter_bits=0)
    with pytest.raises(ValueError, match='maxscore'):
        run(whole, k=15, maxscore=41)
    with pytest.raises(ValueError, match='8..32'):
        run(whole, k=7)


def test_empty_file_raises_what_bqsr_raises(fixture, monkeypatch):
    from kbbq import aln, kmer
    from kbbq.gatk import bqsr
    p = fixture['dir'] / 'empty.sam'
    p.write_text('@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:800\n@RG\tID:g0\tPU:unit0\n')
    bam = aln.AlignmentFile(str(p))
    _no_device(monkeypatch)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    with pytest.raises(StopIteration):
        bqsr.bam_to_kmer_covariates(bam, k=15)


# ---------------------------------------------------------------- the model against the oracle
def test_model_totals_equal_the_reference_based_totals(fixture, oracle):
    """With all flags forced to 0 the model's *_total vectors (and meanq) are those of oracle_bqsr.bam_to_bqsr_covariates on the
    same SAM with no known sites: the reference-based skips are then the soft clips alone (an inserted base is skipped only
    between two known sites, a base before a deletion only when the deletion covers one), which is the model's "outside the
    aligned part".  Clip handling is therefore no obstacle: the whole fixture is compared, clips, indels and all."""
    import _shim
    import oracle_bqsr as OQ
    reads, rgs = fixture['reads'], fixture['rgs']
    fa = _shim.FastaFile(fixture['paths']['fa'])
    ref = {c: fa.fetch(c) for c in fa.references}
    got, info = B.vectors(reads, rgs, 15, use_oq=True, no_errors=True)
    B.check_share(info)                                  # (of the flags before they were forced to 0)
    assert all(int(got[i].sum()) == 0 for i in (1, 3, 5, 7))
    assert any(op == 1 for r in reads for op, _ in r.cigartuples) and any(op == 4 for r in reads for op, _ in r.cigartuples)
    want = OQ.bam_to_bqsr_covariates(reads, rgs, ref, {c: [] for c in ref})
    for i in (0, 2, 4, 6, 8):
        assert np.array_equal(got[i], want[i]), B.VEC[i]
    assert int(got[2].sum()) > 20000
