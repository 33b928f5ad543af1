"""`kbbq benchmark --kmers`, no GPU: the new C ABI symbol and its device-free refusals, the command line's new options, the refusals
of kbbq.benchmark.benchmark_kmers that must come before any device call or collective, and the table and the stderr line from a
hand-written joint array (against the literal text and against tests/kmer_benchmark_model.py)."""
import os

import numpy as np
import pytest

import kmer_benchmark_model as KB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the C ABI
def test_symbol_is_exported_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    assert hasattr(lib, 'kbbq_flag_confusion_dev')
    assert N.PROTOTYPES['kbbq_flag_confusion_dev'] == N.PROTOTYPES['kbbq_count_q_dev']      # three planes, lengths, n, pitch, offset, counts
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    assert ('int kbbq_flag_confusion_dev(kbbq_ctx* ctx, const uint8_t* d_qual, const uint8_t* d_truth, const uint8_t* d_kflags,\n'
            '                            const uint32_t* d_len, int64_t nreads, int pitch, int qoffset, int64_t* d_counts1536);') in header
    assert '#define KBBQ_CONFUSION_MAX_BASES 4294967295ull' in header
    assert N.CONFUSION_MAX_BASES == 4294967295
    assert lib.kbbq_abi_version() == 1


def test_device_free_refusals_of_the_call():
    """No context exists without a device: every answer below is decided on the arguments alone (the stand-in context is never
    dereferenced)."""
    from kbbq import _native as N
    from kbbq import benchmark
    lib = N.load()
    call = lib.kbbq_flag_confusion_dev
    buf = np.zeros(256, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    a = N.ptr(int(base))
    assert call(None, a, a, a, a, 1, 16, 33, a) == N.KBBQ_E_ARG
    assert 'ctx is NULL' in N.last_error()
    for args in ((None, a, a, a, a), (a, None, a, a, a), (a, a, None, a, a), (a, a, a, None, a), (a, a, a, a, None)):
        q, t, k, ln, cnt = args
        assert call(a, q, t, k, ln, 1, 16, 33, cnt) == N.KBBQ_E_ARG
        assert 'kbbq_flag_confusion_dev' in N.last_error() and 'NULL' in N.last_error()
    for pitch in (17, 0, 24, -16):
        assert call(a, a, a, a, a, 1, pitch, 33, a) == N.KBBQ_E_ARG
        assert 'kbbq_flag_confusion_dev: pitch must be a positive multiple of 16' in N.last_error()
    assert call(a, a, a, a, a, -1, 16, 33, a) == N.KBBQ_E_ARG
    assert 'kbbq_flag_confusion_dev: nreads < 0' in N.last_error()
    odd = N.ptr(int(base) + 8)
    assert call(a, odd, a, a, a, 1, 16, 33, a) == N.KBBQ_E_ARG
    assert '16-byte aligned' in N.last_error()
    for qoffset in (-1, 256, -33):
        assert call(a, a, a, a, a, 1, 16, qoffset, a) == N.KBBQ_E_ARG
        assert 'kbbq_flag_confusion_dev: qoffset must be in 0..255, got %d' % qoffset in N.last_error()
    # the launch bound of the 32-bit counters: nreads * pitch <= 2^32 - 1
    for nreads, pitch in (((1 << 28), 16), ((1 << 28) + 1, 16), (1 << 16, 65536), (1 << 40, 160), ((1 << 63) - 1, 16)):
        assert nreads * pitch > benchmark.CONFUSION_BASES_PER_LAUNCH
        assert call(a, a, a, a, a, nreads, pitch, 33, a) == N.KBBQ_E_ARG
        assert 'kbbq_flag_confusion_dev' in N.last_error() and '4294967295 bases per call' in N.last_error()
    assert benchmark.CONFUSION_BASES_PER_LAUNCH == N.CONFUSION_MAX_BASES
    # nothing to do: no launch, no HIP call
    assert call(a, a, a, a, a, 0, 16, 33, a) == N.KBBQ_OK
    assert call(a, a, a, a, a, 0, 65536, 0, a) == N.KBBQ_OK


# ---------------------------------------------------------------- command line
def _patched(monkeypatch):
    from kbbq import benchmark, parallel
    seen = {}
    monkeypatch.setattr(benchmark, 'benchmark', lambda **kw: seen.update(kw))
    monkeypatch.setattr(parallel, 'init_from_env', lambda: None)
    return seen


def test_argparse_kmers_reaches_the_benchmark(monkeypatch):
    from kbbq import main
    seen = _patched(monkeypatch)
    main.main(['benchmark', '-b', 'x.sam', '-r', 'x.fa', '-v', 'x.vcf', '--kmers'])
    assert seen == dict(bamfile='x.sam', fafile='x.fa', vcffile='x.vcf', fastqfile=None, label=None, use_oq=False, bedfh=None,
                        kmers=dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4))
    seen.clear()
    main.main(['benchmark', '-b', 'x.sam', '-r', 'x.fa', '-v', 'x.vcf', '--kmers', '-k', '21', '--min-count', '3', '--slots', '4096',
               '--prefilter', '--filter-bits', '8', '-u', '-l', 'lbl'])
    assert seen['kmers'] == dict(k=21, min_count=3, slots=4096, prefilter=True, filter_bits=8)
    assert seen['use_oq'] is True and seen['label'] == 'lbl'


def test_argparse_old_form_is_unchanged(monkeypatch):
    from kbbq import main
    seen = _patched(monkeypatch)
    main.main(['benchmark', '-b', 'x.sam', '-r', 'x.fa', '-v', 'x.vcf', '-f', 'x.fq', '-l', 'lbl', '-u'])
    assert seen == dict(bamfile='x.sam', fafile='x.fa', vcffile='x.vcf', fastqfile='x.fq', label='lbl', use_oq=True, bedfh=None)


_OLD = ['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf']


@pytest.mark.parametrize('argv,message', [
    (_OLD + ['--kmers', '-f', 'x.fq'], '-f/--fastq: not with --kmers'),
    (_OLD + ['-k', '21'], '-k/--kmer: only with --kmers'),
    (_OLD + ['--min-count', '3'], '--min-count: only with --kmers'),
    (_OLD + ['--slots', '1024'], '--slots: only with --kmers'),
    (_OLD + ['--prefilter'], '--prefilter: only with --kmers'),
    (_OLD + ['--filter-bits', '4'], '--filter-bits: only with --kmers'),
    (_OLD + ['-f', 'x.fq', '--prefilter', '--filter-bits', '4'], '--prefilter, --filter-bits: only with --kmers'),
    (['benchmark', '-b', 'x', '-r', 'x.fa', '--kmers'], 'required'),
])
def test_argparse_refuses(monkeypatch, argv, message, capsys):
    from kbbq import main
    seen = _patched(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(argv)
    assert exc.value.code == 2 and not seen
    assert message in capsys.readouterr().err


# ---------------------------------------------------------------- refusals before any device call
def _no_device(monkeypatch):
    """Every way to the device and every collective raise: a refusal that arrives anyway came first."""
    from kbbq import _device, _native, benchmark, kmer, parallel

    def boom(*a, **kw):
        raise AssertionError('a device call was made')

    def collective(*a, **kw):
        raise AssertionError('a collective was started')
    monkeypatch.setattr(kmer, '_ctx', boom)
    monkeypatch.setattr(_native, 'load', boom)
    monkeypatch.setattr(_device, '_torch', boom)
    monkeypatch.setattr(_device, 'context', boom)
    for name in ('prefilter_kmers', 'count_kmers', 'flag_errors', 'kmer_histogram'):
        monkeypatch.setattr(kmer, name, boom)
    for name in ('_Genome', '_flag_batch', '_qual_chars_dev', 'kmer_confusion'):
        monkeypatch.setattr(benchmark, name, boom)
    for name in ('all_gather_object', 'sum_over_ranks', 'max_over_ranks', 'raise_first_error', 'barrier', 'all_to_all_rows',
                 'allreduce_tables', 'broadcast_object', 'all_gather_rows'):
        monkeypatch.setattr(parallel, name, collective)


@pytest.fixture(scope='module')
def truthset(tmp_path_factory):
    import oracle_benchmark as OB
    return OB.synth_truthset(str(tmp_path_factory.mktemp('benchmark_kmers_host')), 3, npairs=10)


def test_ranks_are_refused_before_any_collective(truthset, monkeypatch):
    from kbbq import aln, benchmark, kmer
    bam = aln.AlignmentFile(truthset['sam'])
    _no_device(monkeypatch)
    for rank in (0, 1):                                  # every rank refuses, not rank 0 alone
        monkeypatch.setattr(kmer, '_ranks', lambda rank=rank: (2, rank))
        with pytest.raises(ValueError, match=r'benchmark --kmers does not run across ranks.*on one GPU'):
            benchmark.benchmark_kmers(bam, None, None, k=15)
        with pytest.raises(ValueError, match='one GPU'):
            benchmark.benchmark_kmers(bam, None, None, k=15, prefilter=True, min_count=1)


def test_argument_refusals_come_before_any_device_call(truthset, monkeypatch):
    from kbbq import aln, benchmark, kmer
    bam = aln.AlignmentFile(truthset['sam'])
    _no_device(monkeypatch)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    run = lambda *a, **kw: benchmark.benchmark_kmers(bam, None, None, *a, **kw)
    for k in (7, 33, 0):
        with pytest.raises(ValueError, match=r'k must be in 8\.\.32, got %d' % k):
            run(k=k)
    for mc in (0, -2):
        with pytest.raises(ValueError, match='min_count must be >= 1, got %d' % mc):
            run(k=15, min_count=mc)
    with pytest.raises(ValueError, match='min_count must be >= 2 with the prefilter, got 1'):
        run(k=15, prefilter=True, min_count=1)
    with pytest.raises(ValueError, match='filter_bits'):
        run(k=15, prefilter=True, filter_bits=0)
    import _shim
    for other in (list(_shim.AlignmentFile(truthset['sam'])), truthset['sam'], None):
        with pytest.raises(TypeError, match='benchmark_kmers takes a kbbq.aln.AlignmentFile'):
            benchmark.benchmark_kmers(other, None, None, k=15)
    with pytest.raises(ValueError, match='not a FASTQ'):
        benchmark.benchmark(truthset['sam'], truthset['fa'], truthset['vcf'], fastqfile=truthset['fq'], kmers=dict(k=15))


# ---------------------------------------------------------------- the table and the stderr line
def _hand_written():
    J = np.zeros((256, 2, 3), dtype=np.int64)
    J[2] = [[90, 1, 2], [3, 4, 0]]                     # 100 bases, 7 errors, 5 flagged (4 of them errors), 2 unresolved
    J[30] = [[0, 0, 5], [0, 0, 1]]                     # every base unresolved: kmer_q_skip is 0
    J[41] = [[99990, 0, 0], [0, 10, 0]]                # 100,000 bases, 10 errors, all flagged
    J[255] = [[7, 0, 0], [0, 0, 0]]                    # no error and nothing flagged: p = 0 -> 42
    return J


TABLE = ('#predicted_q\tbases\terrors\tflagged\tflagged_errors\tunresolved\tunresolved_errors\tactual_q\tkmer_q\tkmer_q_skip\tlabel\n'
         '2\t100\t7\t5\t4\t2\t0\t11\t13\t12\tlbl\n'
         '30\t6\t1\t0\t0\t6\t1\t7\t42\t0\tlbl\n'
         '41\t100000\t10\t10\t10\t0\t0\t40\t40\t40\tlbl\n'
         '255\t7\t0\t0\t0\t0\t0\t42\t42\t42\tlbl\n')


def test_table_from_a_hand_written_joint_array(capsys):
    from kbbq import benchmark
    J = _hand_written()
    benchmark.print_benchmark_kmers(J, 'lbl')
    out = capsys.readouterr().out
    assert out == TABLE
    assert out == KB.render(J, 'lbl')
    benchmark.print_benchmark_kmers(np.zeros((256, 2, 3), dtype=np.int64), 'x')
    assert capsys.readouterr().out == TABLE.split('\n')[0] + '\n'


def test_summary_line():
    from kbbq import benchmark
    J = _hand_written()
    t = benchmark.kmer_totals(J)
    assert t == KB.totals(J) == dict(bases=100113, errors=18, flagged=15, flagged_errors=14, unresolved=8, unresolved_errors=1)
    info = dict(k=21, min_count=3, reads=9, slots=2048, prefilter=False, admitted=None, **t)
    line = ('kbbq benchmark: k=21 min_count=3 reads=9 bases=100113 errors=18 flagged=15 flagged_errors=14 unresolved=8 '
            'unresolved_errors=1 precision=0.9333 recall=0.7778')
    assert benchmark.kmer_summary(info) == line == KB.summary(info)
    info.update(prefilter=True, admitted=77)
    assert benchmark.kmer_summary(info) == line + ' prefilter=1 admitted=77 slots=2048' == KB.summary(info, prefilter=(77, 2048))
    zero = dict(k=15, min_count=0, reads=0, slots=0, prefilter=False, admitted=None, **benchmark.kmer_totals(np.zeros((256, 2, 3))))
    assert benchmark.kmer_summary(zero).endswith('unresolved_errors=0 precision=0.0000 recall=0.0000')
