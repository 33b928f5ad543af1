"""`--partitions P|auto` of kbbq correct / recalibrate -c / bqsr --kmers / benchmark --kmers, no GPU: the CPU model of the rounds
(tests/kmer_partition_model.py) against tests/kmer_model.py on the whole input, the owner function on the host against an
independent restatement, the six new C ABI symbols and their device-free refusals, the arithmetic of the table sizes, the command
line's new option on the four commands, its refusal in a process group before any device call or collective, and the stderr
lines."""
import os
import re

import numpy as np
import pytest

import kmer_model as M
import kmer_partition_model as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the model
def test_the_fixture_is_the_one_the_figures_are_of():
    seq, meta = PT.fixture()
    assert seq.shape[0] == 3571
    for k, (windows, distinct, twice, t) in PT.FIGURES.items():
        keys, counts = PT.counted(k)
        lens = meta.astype(np.int64)
        assert int(np.maximum(lens - k + 1, 0).sum()) == windows
        assert int(M.windows(seq, meta, k)[2].sum()) == int(counts.sum()) <= windows        # (an N breaks the windows over it)
        assert (keys.size, int((counts >= 2).sum()), M.threshold(M.histogram(counts))) == (distinct, twice, t)


@pytest.mark.parametrize('k', (21, 31))
@pytest.mark.parametrize('P', (2, 3, 8, 64))
def test_rounds_add_up_to_the_one_table(k, P):
    keys, counts = PT.counted(k)
    t = PT.FIGURES[k][3]
    hist, kept_keys, kept_counts, largest = PT.rounds(keys, counts, P, 2)
    assert np.array_equal(hist, M.histogram(counts))                      # the sum of the rounds' histograms
    assert M.threshold(hist) == t
    solid = counts >= t                                                   # the union filtered at t is the solid set
    assert np.array_equal(kept_keys[kept_counts >= t], keys[solid]) and np.array_equal(kept_counts[kept_counts >= t], counts[solid])
    assert kept_keys.size == PT.FIGURES[k][2]                             # ... and all of it the keys of count >= 2
    owner = PT.part(keys, P)
    assert owner.min() >= 0 and owner.max() < P
    sizes = np.bincount(owner, minlength=P)
    assert int(sizes.sum()) == keys.size and int(sizes.max()) == largest
    if k in PT.LARGEST:
        assert largest == PT.LARGEST[k][P]
    # with min_count given, keep = min_count: nothing below it is kept, everything at or above it is
    _, kk, kc, _ = PT.rounds(keys, counts, P, t + 1)
    assert np.array_equal(kk, keys[counts >= t + 1]) and np.array_equal(kc, counts[counts >= t + 1])


def test_owner_on_the_host_is_the_restatement():
    from kbbq import _native as N
    from kbbq import kmer
    lib = N.load()
    rng = np.random.default_rng(17)
    keys = np.concatenate([rng.integers(0, 1 << 63, 100000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 100000, dtype=np.uint64),
                           np.array([0, 1, (1 << 64) - 2], dtype=np.uint64)])
    for P in (1, 2, 3, 8, 64, 1024):
        want = PT.part(keys, P)
        assert np.array_equal(kmer.owner(keys, P).astype(np.int64), want)
        assert want.min() >= 0 and want.max() < P
        some = np.concatenate([np.arange(0, keys.size, 997), np.arange(keys.size - 3, keys.size)])
        for i in some.tolist():
            assert int(lib.kbbq_kmer_owner(int(keys[i]), P)) == PT.part_int(int(keys[i]), P) == int(want[i])
    for P in (2, 3, 64):                                                  # ... the C statement on all of them, once per P
        got = np.array([lib.kbbq_kmer_owner(int(x), P) for x in keys[::10].tolist() + keys[-3:].tolist()], dtype=np.int64)
        assert np.array_equal(got, np.concatenate([PT.part(keys[::10], P), PT.part(keys[-3:], P)]))


def test_c_owner_on_every_key():
    from kbbq import _native as N
    lib = N.load()
    rng = np.random.default_rng(18)
    keys = rng.integers(0, 1 << 63, 100000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 100000, dtype=np.uint64)
    fn = lib.kbbq_kmer_owner
    got = np.fromiter((fn(x, 8) for x in keys.tolist()), dtype=np.int64, count=keys.size)
    assert np.array_equal(got, PT.part(keys, 8))


# ---------------------------------------------------------------- the C ABI
SIBLINGS = {'kbbq_kmer_count_part_dev': 'kbbq_kmer_count_dev', 'kbbq_kmer_count_filtered_part_dev': 'kbbq_kmer_count_filtered_dev',
            'kbbq_kmer_count_part': 'kbbq_kmer_count', 'kbbq_kmer_count_filtered_part': 'kbbq_kmer_count_filtered',
            'kbbq_kmer_count_rows_part_dev': 'kbbq_kmer_count_rows_dev',
            'kbbq_kmer_count_filtered_rows_part_dev': 'kbbq_kmer_count_filtered_rows_dev'}


def test_symbols_are_exported_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    for name, sibling in SIBLINGS.items():
        assert hasattr(lib, name)
        ret, args = N.PROTOTYPES[sibling]
        assert N.PROTOTYPES[name] == (ret, args + [ret, ret])             # the sibling's arguments, `int parts` and `int part`
        m = re.search(r'^int %s\(kbbq_ctx\* ctx, kbbq_kmer_table\* table,[^;]*int parts,\s+int part\);' % name, header, flags=re.M)
        assert m, name
    assert lib.kbbq_abi_version() == 1
    assert re.search(r'^#define KBBQ_ABI_VERSION 1$', header, flags=re.M)


def _calls():
    """name -> call(ctx, table, filter, seq, meta, n, pitch, parts, part) with the arguments each call has."""
    from kbbq import _native as N
    lib = N.load()
    return {
        'kbbq_kmer_count_part_dev': lambda c, t, f, s, m, n, pitch, P, p: lib.kbbq_kmer_count_part_dev(c, t, s, m, n, pitch, P, p),
        'kbbq_kmer_count_filtered_part_dev':
            lambda c, t, f, s, m, n, pitch, P, p: lib.kbbq_kmer_count_filtered_part_dev(c, t, f, s, m, n, pitch, P, p),
        'kbbq_kmer_count_part': lambda c, t, f, s, m, n, pitch, P, p: lib.kbbq_kmer_count_part(c, t, s, m, n, pitch, P, p),
        'kbbq_kmer_count_filtered_part':
            lambda c, t, f, s, m, n, pitch, P, p: lib.kbbq_kmer_count_filtered_part(c, t, f, s, m, n, pitch, P, p),
        'kbbq_kmer_count_rows_part_dev':
            lambda c, t, f, s, m, n, pitch, P, p, flags=0: lib.kbbq_kmer_count_rows_part_dev(c, t, s, m, n, pitch, flags, P, p),
        'kbbq_kmer_count_filtered_rows_part_dev':
            lambda c, t, f, s, m, n, pitch, P, p, flags=0: lib.kbbq_kmer_count_filtered_rows_part_dev(c, t, f, s, m, n, pitch, flags, P, p),
    }


def test_device_free_refusals_of_the_calls():
    """No context, table or filter exists without a device: the pointers below are never dereferenced, every refusal is decided
    on the arguments alone."""
    import ctypes
    from kbbq import _native as N
    buf = np.zeros(256, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16                      # 16-byte aligned inside buf
    fake, plane, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 64), ctypes.c_void_p(base + 64 + 4)
    for name, call in _calls().items():
        host = not name.endswith('_dev')
        for P, p in ((0, 0), (1025, 0), (-1, 0), (2, -1), (2, 2), (1, 1), (1024, 1024)):
            # before anything else, whatever the other arguments are
            assert call(None, None, None, None, None, -5, 17, P, p) == N.KBBQ_E_ARG, (name, P, p)
            err = N.last_error()
            assert name + ':' in err and ('parts must be in 1..1024' in err if not 1 <= P <= 1024 else 'part must be in 0..%d' % (P - 1) in err)
        for P, p in ((1, 0), (2, 1), (1024, 1023)):                      # the siblings' refusals stay, parts = 1 included
            assert call(None, None, None, None, None, 0, 16, P, p) == N.KBBQ_E_ARG
            assert name + ':' in N.last_error() and 'NULL' in N.last_error()
            assert call(fake, None, fake, plane, plane, 1, 16, P, p) == N.KBBQ_E_ARG and 'NULL' in N.last_error()
            if 'filtered' in name:
                assert call(fake, fake, None, plane, plane, 1, 16, P, p) == N.KBBQ_E_ARG
                assert name + ':' in N.last_error() and 'NULL' in N.last_error() and 'filter' in N.last_error()
            for pitch in (24, 0, -16, 17):
                assert call(fake, fake, fake, plane, plane, 1, pitch, P, p) == N.KBBQ_E_ARG
                assert name + ':' in N.last_error() and 'pitch' in N.last_error()
            assert call(fake, fake, fake, None, plane, 1, 16, P, p) == N.KBBQ_E_ARG               # NULL plane
            assert name + ':' in N.last_error() and 'NULL plane' in N.last_error()
            assert call(fake, fake, fake, plane, None, 1, 16, P, p) == N.KBBQ_E_ARG               # NULL meta
            assert name + ':' in N.last_error() and 'NULL plane' in N.last_error()
            assert call(fake, fake, fake, plane, plane, -1, 16, P, p) == N.KBBQ_E_ARG
            assert name + ':' in N.last_error()
            if not host:                                                  # a host buffer has no alignment to keep
                assert call(fake, fake, fake, off, plane, 1, 16, P, p) == N.KBBQ_E_ARG
                assert name + ':' in N.last_error() and 'aligned' in N.last_error()
            if 'rows' in name:
                assert call(fake, fake, fake, off, plane, 1, 16, P, p, N.ROWS_NIBBLES) == N.KBBQ_E_ARG
                assert name + ':' in N.last_error() and '8-byte aligned' in N.last_error()
                for flags in (8, N.ROWS_TWINS):
                    assert call(fake, fake, fake, plane, plane, 1, 16, P, p, flags) == N.KBBQ_E_ARG
                    assert name + ':' in N.last_error()


def test_python_refuses_a_partition_outside_its_range_before_any_device_call(monkeypatch):
    from kbbq import _native, kmer

    def never(*a, **kw):
        raise AssertionError('a device call')
    monkeypatch.setattr(_native, 'load', never)
    monkeypatch.setattr(kmer, '_ctx', never)
    plane, meta = np.zeros((1, 16), dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    for parts, part in ((0, 0), (1025, 0), (2, 2), (2, -1)):
        for call in (lambda: kmer.count_kmers(plane, meta, parts=parts, part=part),
                     lambda: kmer.count_batch(None, parts=parts, part=part)):
            with pytest.raises(ValueError, match='parts? must be in'):
                call()


# ---------------------------------------------------------------- arithmetic
@pytest.mark.parametrize('good', (1, 2, 64, 'auto', 3.0, np.int64(8)))
def test_check_partitions_accepts(good):
    from kbbq import kmer
    got = kmer.check_partitions(good)
    assert got == good and (got == 'auto' or type(got) is int)


@pytest.mark.parametrize('bad', (0, 65, -1, 2.5, True, False, 'x', '2', 'AUTO', None, [2]))
def test_check_partitions_refuses(bad):
    from kbbq import kmer
    with pytest.raises(ValueError, match=r"partitions must be an integer in 1\.\.64 or 'auto'"):
        kmer.check_partitions(bad)


def test_table_sizes_follow_the_formulas():
    """By hand, for F's 492,313 windows at k = 31 (12 bytes a slot, load factor 0.5, powers of two from 1024):
    P = 1: 492,313 keys want 2^20 slots = 12,582,912 bytes.
    P = 2: ceil(492,313 x 9 / 16) = 276,927 -> 2^20.    P = 3: ceil(.. / 24) = 184,618 -> 2^19 = 6,291,456 bytes.
    P = 8: ceil(.. / 64) = 69,232 -> 2^18.    P = 33: 16,784 -> 2^16;  P = 34: 16,290 -> 2^15 = 393,216 bytes, as P = 64 (8,654)."""
    from kbbq import kmer
    W = PT.FIGURES[31][0]
    assert [kmer.partition_windows(W, P) for P in (2, 3, 8, 33, 34, 64)] == [276927, 184618, 69232, 16784, 16290, 8654]
    big = 1 << 34
    assert kmer.default_slots(W, big) == 1 << 20
    assert [kmer.partition_slots(W, P, big) for P in (2, 3, 8, 33, 34, 64)] == [1 << 20, 1 << 19, 1 << 18, 1 << 16, 1 << 15, 1 << 15]
    assert kmer.partition_slots(W, 8, 1 << 20) == 1 << 15                 # capped by HALF the budget: 2^15 x 12 <= 524,288 < 2^16 x 12
    assert kmer.partition_slots(1, 64, big) == kmer.MIN_SLOTS
    # partitions_for: the smallest P whose table fits half the budget
    assert kmer.partitions_for(W, 2 * 12582912) == 1                      # exactly fits
    assert kmer.partitions_for(W, 2 * 12582912 - 1) == 3                  # 2 partitions want 2^20 slots too
    assert kmer.partitions_for(W, 2 * 6291456 - 1) == 5                   # ceil(.. / 40) = 110,771 -> 2^18
    assert kmer.partitions_for(W, 2 * 393216) == 34
    assert kmer.partitions_for(W, 2 * 393216 + 1) == 34
    assert kmer.partitions_for(0, 1 << 20) == 1
    with pytest.raises(ValueError, match='KBBQ_DEVICE_BUDGET'):
        kmer.partitions_for(W, 2 * 393216 - 1)
    assert kmer.resolve_partitions('auto', W, 2 * 12582912 - 1) == 3 and kmer.resolve_partitions(7, W, 1) == 7


# ---------------------------------------------------------------- command line
def _no_ranks(monkeypatch):
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the commands then leave the memory back end alone


@pytest.mark.parametrize('argv, message', (
    (['recalibrate', '-f', 'a.fq', 'b.fq', '--partitions', '2'], '--partitions: only with -c/--correct'),
    (['recalibrate', '-b', 'a.bam', '--partitions', 'auto'], '--partitions: only with -c/--correct'),
    (['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--partitions', '2'], '--partitions: only with --kmers'),
    (['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '--partitions', '2'], '--partitions: only with --kmers'),
))
def test_partitions_only_with_the_k_mer_form(monkeypatch, capsys, argv, message):
    from kbbq import benchmark as bm, main, recalibrate as recal
    from kbbq.gatk import bqsr
    _no_ranks(monkeypatch)
    monkeypatch.setattr(recal, 'recalibrate', lambda **kw: pytest.fail('ran'))
    monkeypatch.setattr(bm, 'benchmark', lambda **kw: pytest.fail('ran'))
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: pytest.fail('ran'))
    with pytest.raises(SystemExit) as exc:
        main.main(argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


@pytest.mark.parametrize('command', (['correct', '-f', 'x.fq'], ['recalibrate', '-c', 'x.fq'], ['bqsr', '-b', 'x', '--kmers', '-g', 'r'],
                                     ['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '--kmers']))
@pytest.mark.parametrize('value', ('0', '65', '-1', 'two', '2.5', 'Auto'))
def test_values_outside_the_range_are_argparse_errors(monkeypatch, capsys, command, value):
    from kbbq import main
    _no_ranks(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(command + ['--partitions', value])
    assert exc.value.code == 2
    assert 'argument --partitions' in capsys.readouterr().err


def test_the_option_reaches_the_four_commands_only_when_given(monkeypatch):
    from kbbq import aln, benchmark as bm, kmer, main, recalibrate as recal
    from kbbq.gatk import bqsr
    _no_ranks(monkeypatch)
    seen = []
    monkeypatch.setattr(kmer, 'main_correct', lambda path, **kw: seen.append(kw))
    for more in ([], ['--partitions', '1'], ['--partitions', '3'], ['--partitions', 'auto', '--prefilter', '--passes', '2']):
        main.main(['correct', '-f', 'x.fq'] + more)
    assert [kw.get('partitions') for kw in seen] == [None, 1, 3, 'auto'] and 'partitions' not in seen[0]
    assert seen[3]['prefilter'] is True and seen[3]['passes'] == 2

    del seen[:]
    checked = []
    monkeypatch.setattr(recal, 'check_corrected', lambda *a, **kw: checked.append(kw))
    monkeypatch.setattr(recal, 'recalibrate_corrected',
                        lambda path, **kw: seen.append(kw) or dict(k=kw['k'], min_count=3, reads=5, changed_bases=7, admitted=11, slots=16))
    for more in ([], ['--partitions', '4'], ['--partitions', 'auto']):
        main.main(['recalibrate', '-c', 'x.fq'] + more)
    assert [kw.get('partitions') for kw in seen] == [None, 4, 'auto'] and 'partitions' not in seen[0]
    assert checked == [{}, dict(partitions=4), dict(partitions='auto')]    # refused, where it is, before the process group exists

    del seen[:]

    class _Report:
        def write(self, path):
            pass

    def kmers(bam, **kw):
        seen.append(kw)
        kw['info'].update(k=kw['k'], min_count=7, reads=5, flagged_bases=11, skipped_bases=17, admitted=13, slots=1024)
        return _Report()
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: 'opened:' + p)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', kmers)
    for more in ([], ['--partitions', '2', '--skip-unresolved']):
        main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp'] + more)
    assert 'partitions' not in seen[0] and seen[1]['partitions'] == 2 and seen[1]['skip_unresolved'] is True

    del seen[:]
    monkeypatch.setattr(bm, 'benchmark', lambda **kw: seen.append(kw))
    for more in ([], ['--partitions', '5']):
        main.main(['benchmark', '-b', 'x.sam', '-r', 'x.fa', '-v', 'x.vcf', '--kmers'] + more)
    assert 'partitions' not in seen[0]['kmers'] and seen[1]['kmers'] == dict(seen[0]['kmers'], partitions=5)


def test_the_keyword_goes_down_only_when_it_is_not_1(monkeypatch):
    from kbbq import kmer
    from kbbq.gatk import bqsr
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    got = []

    def fake(path, out, **kw):
        got.append(kw)
        return dict(k=kw['k'], min_count=4, reads=9, changed=np.array([1, 2]))
    monkeypatch.setattr(kmer, 'correct_fastq', fake)
    for P in (1, 2, 'auto'):
        kmer.main_correct('x.fq', partitions=P)
    assert [kw.get('partitions') for kw in got] == [None, 2, 'auto']      # partitions = 1 takes exactly the call without it
    seen = {}
    monkeypatch.setattr(bqsr.utils, 'get_rg_to_pu', lambda bam: {'g0': 'unit0'})
    monkeypatch.setattr(bqsr, 'bam_to_kmer_covariates', lambda bam, **kw: seen.update(kw=kw) or 'vectors')
    monkeypatch.setattr(bqsr, 'vectors_to_report', lambda *a: a)
    bqsr.bam_to_report_kmers('bam', k=15, partitions=2)
    assert seen['kw']['partitions'] == 2
    bqsr.bam_to_report_kmers('bam', k=15)
    assert 'partitions' not in seen['kw']


# ---------------------------------------------------------------- a process group
def _no_device(monkeypatch):
    """The library, the context and every collective raise: a refusal that arrives anyway came first."""
    from kbbq import _native, kmer, parallel

    def boom(*a, **kw):
        raise AssertionError('a device call was made')

    def collective(*a, **kw):
        raise AssertionError('a collective was started')
    monkeypatch.setattr(kmer, '_ctx', boom)
    monkeypatch.setattr(_native, 'load', boom)
    for name in ('prefilter_kmers', 'count_kmers', 'count_batch', 'flag_errors', 'kmer_histogram', 'count_partitioned', 'select', 'merge',
                 'count_block', 'count_rounds'):
        monkeypatch.setattr(kmer, name, boom)
    for name in ('all_gather_object', 'sum_over_ranks', 'max_over_ranks', 'raise_first_error', 'barrier', 'all_to_all_rows',
                 'allreduce_tables', 'broadcast_object', 'all_gather_rows'):
        monkeypatch.setattr(parallel, name, collective)


REFUSAL = r'partitions do not run across ranks.*owner tables.*already split.*--local-slots'


@pytest.mark.parametrize('P', (2, 64, 'auto'))
def test_a_process_group_refuses_partitions_before_any_collective(monkeypatch, P):
    from kbbq import benchmark as bm, kmer, recalibrate as recal
    from kbbq.gatk import bqsr
    _no_device(monkeypatch)
    plane, meta = np.zeros((1, 16), dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    for rank in (0, 1):                                  # every rank refuses, not rank 0 alone
        monkeypatch.setattr(kmer, '_ranks', lambda rank=rank: (2, rank))
        for call in (lambda: kmer.main_correct('x.fq', partitions=P),
                     lambda: kmer.correct_fastq('x.fq', 'y.fq', partitions=P),
                     lambda: kmer.correct_reads(plane, meta, partitions=P),
                     lambda: recal.recalibrate_corrected('x.fq', partitions=P),
                     lambda: recal.check_corrected('x.fq', partitions=P),
                     lambda: bqsr.bam_to_kmer_covariates(None, partitions=P),
                     lambda: bm.benchmark_kmers(None, None, None, partitions=P)):
            with pytest.raises(ValueError, match=REFUSAL):
                call()
    # under a launcher whose group does not exist yet, recalibrate -c refuses on the environment
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    monkeypatch.setattr(recal.parallel, 'launched_from_env', lambda: True)
    with pytest.raises(ValueError, match=REFUSAL):
        recal.check_corrected('x.fq', partitions=P)


def test_a_process_group_takes_partitions_1_as_before(monkeypatch):
    """partitions = 1 is no option at all: the rank path's own refusals and calls come, not the new one."""
    from kbbq import kmer
    from kbbq.gatk import bqsr
    _no_device(monkeypatch)
    monkeypatch.setattr(kmer, '_ranks', lambda: (2, 0))
    with pytest.raises(ValueError, match=r'bqsr -r -v.*under ranks'):
        bqsr.bam_to_kmer_covariates(None, k=15, partitions=1)
    monkeypatch.setattr(kmer, 'correct_fastq_ranks', lambda *a, **kw: (_ for _ in ()).throw(KeyError('the rank path')))
    with pytest.raises(KeyError, match='the rank path'):
        kmer.main_correct('x.fq', partitions=1)


# ---------------------------------------------------------------- stderr
def test_correct_summary_line(monkeypatch, capsys):
    from kbbq import kmer
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    resolved = {}

    def fake(path, out, **kw):
        info = dict(k=kw['k'], min_count=4, reads=9, changed=np.array([1, 2]), admitted=5, slots=32)
        P = resolved.get(kw.get('partitions', 1), kw.get('partitions', 1))
        if P > 1:
            info.update(partitions=P, kept_pairs=10, solid_slots=1024)
        return info
    monkeypatch.setattr(kmer, 'correct_fastq', fake)
    kmer.main_correct('x.fq')
    kmer.main_correct('x.fq', partitions=1)
    kmer.main_correct('x.fq', partitions=3)
    kmer.main_correct('x.fq', partitions=3, passes=2, fix_n=True)
    kmer.main_correct('x.fq', partitions=8, passes=3, fix_n=True, prefilter=True)
    resolved['auto'] = 1
    kmer.main_correct('x.fq', partitions='auto', prefilter=True)
    resolved['auto'] = 5
    kmer.main_correct('x.fq', partitions='auto')
    assert capsys.readouterr().err.splitlines() == [
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 partitions=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 fix_n=1 passes=2 partitions=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 fix_n=1 passes=3 partitions=8 prefilter=1 admitted=5 slots=32',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 prefilter=1 admitted=5 slots=32',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 partitions=5']


def test_recalibrate_and_bqsr_summary_lines(monkeypatch, capsys):
    from kbbq import aln, main, recalibrate as recal
    from kbbq.gatk import bqsr
    _no_ranks(monkeypatch)
    monkeypatch.setattr(recal, 'check_corrected', lambda *a, **kw: None)

    def fake(path, **kw):
        info = dict(k=kw['k'], min_count=3, reads=5, changed_bases=7, admitted=11, slots=16, skipped_bases=2)
        if kw.get('partitions', 1) not in (1, 'auto'):
            info.update(partitions=kw['partitions'])
        return info
    monkeypatch.setattr(recal, 'recalibrate_corrected', fake)
    main.main(['recalibrate', '-c', 'x.fq', '--partitions', '1'])
    main.main(['recalibrate', '-c', 'x.fq', '--partitions', 'auto'])                                  # resolved to 1
    main.main(['recalibrate', '-c', 'x.fq', '--partitions', '3'])
    main.main(['recalibrate', '-c', 'x.fq', '--partitions', '3', '--skip-unresolved', '--fix-n', '--passes', '2', '--prefilter'])
    lines = [x for x in capsys.readouterr().err.splitlines() if x.startswith('kbbq recalibrate:')]
    assert lines == ['kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 partitions=3',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 skipped_bases=2 fix_n=1 passes=2 partitions=3 '
                     'prefilter=1 admitted=11 slots=16']

    class _Report:
        def write(self, path):
            pass

    def kmers(bam, **kw):
        kw['info'].update(k=kw['k'], min_count=7, reads=5, flagged_bases=11, admitted=13, slots=1024, skipped_bases=17)
        if kw.get('partitions', 1) not in (1, 'auto'):
            kw['info'].update(partitions=kw['partitions'])
        return _Report()
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: 'opened:' + p)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', kmers)
    base = ['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp']
    main.main(base + ['--partitions', 'auto'])
    main.main(base + ['--partitions', '2'])
    main.main(base + ['--partitions', '2', '--passes', '3', '--skip-unresolved', '--prefilter'])
    assert capsys.readouterr().err.splitlines() == [
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11',
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11 partitions=2',
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11 skipped_bases=17 passes=3 partitions=2 prefilter=1 admitted=13 slots=1024']


def test_benchmark_summary_line():
    from kbbq import benchmark as bm
    info = dict(k=31, min_count=4, reads=9, bases=100, errors=10, flagged=8, flagged_errors=8, unresolved=5, unresolved_errors=1,
                prefilter=False, admitted=None, slots=64)
    line = ('kbbq benchmark: k=31 min_count=4 reads=9 bases=100 errors=10 flagged=8 flagged_errors=8 unresolved=5 '
            'unresolved_errors=1 precision=1.0000 recall=0.8000')
    assert bm.kmer_summary(info) == bm.kmer_summary(dict(info, partitions=1)) == line
    assert bm.kmer_summary(dict(info, partitions=4)) == line + ' partitions=4'
    assert bm.kmer_summary(dict(info, passes=3, partitions=4, prefilter=True, admitted=7)) \
        == line + ' passes=3 partitions=4 prefilter=1 admitted=7 slots=64'
