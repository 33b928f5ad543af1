"""`--passes P` of kbbq correct / recalibrate -c / bqsr --kmers / benchmark --kmers, no GPU: the CPU model of the repeated rule
(tests/kmer_passes_model.py) against figures worked out independently and against hand-built rows whose passes are known by
construction, the command line's new option on the four commands, and the four new C ABI symbols."""
import os
import re

import numpy as np
import pytest

import kmer_model as M
import kmer_passes_model as PM
import kmer_unresolved_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the model
# (k, t): per pass, (changed bases -- all of them to the truth --, unresolved bases) of synth(11, ...) below
TABLE = {
    (21, 6): [(1149, 6256), (1206, 629), (1215, 379), (1216, 292)],
    (31, 5): [(1078, 11497), (1189, 1376), (1204, 582), (1205, 427)],
}


@pytest.mark.parametrize('k', (21, 31))
def test_model_reproduces_the_worked_table(k):
    seq, meta, truth, errs = M.synth(11, genome_len=4000, depth=30, err=0.01, len_lo=100, len_hi=150)
    assert int(meta.sum()) == 120503 and int(errs.sum()) == 1224
    (t, want), = [(kt[1], v) for kt, v in TABLE.items() if kt[0] == k]
    solid, got_t = PM.solid_set(seq, meta, k)
    assert got_t == t                                    # the first valley of the reads as read
    steps = PM.trace(seq, meta, k, t, 4, solid_keys=solid)
    for (changed, unresolved), (plane, ch, flags, _) in zip(want, steps):
        differs = plane != seq
        assert int(ch.sum()) == int(differs.sum()) == changed
        assert np.array_equal(plane[differs], truth[differs])           # precision does not move: every change is to the truth
        assert int((flags == 2).sum()) == unresolved
        assert not ((flags == 2) & differs).any() and np.array_equal(flags == 1, differs)
    # pass 1 is the one-pass rule of the other models
    one, changed, _ = M.correct(seq, meta, k, t)
    assert np.array_equal(steps[0][0], one) and np.array_equal(steps[0][1], changed)
    cls = U.classify(seq, meta, k, t)[0]
    assert np.array_equal(steps[0][2], cls)


@pytest.fixture(scope='module')
def hand():
    seq, meta, cases = PM.hand_rows()
    steps = PM.trace(seq, meta, PM.HAND_K, PM.HAND_T, 8)
    return seq, meta, cases, steps


def _row(steps, P, row):
    plane, changed, flags, ran = steps[P - 1]
    return plane[row], int(changed[row]), flags[row, :PM.HAND_LEN].tolist(), int(ran[row])


def test_the_tiles_are_trusted_and_stop_after_one_pass(hand):
    seq, meta, cases, steps = hand
    first = min(row for row, _ in cases.values())
    for plane, changed, flags, ran in steps:
        assert np.array_equal(plane[:first], seq[:first]) and not changed[:first].any() and not flags[:first].any()
        assert (ran[:first] == 1).all()


@pytest.mark.parametrize('name, L', (('two_pass', 0), ('two_pass_end', PM.HAND_LEN - 1)))
def test_two_pass_case(hand, name, L):
    """Errors at bases 2 and 8 from an end of the read, k = 11: pass 1 corrects the inner one, pass 2 the outer one, and the bases
    between them go from 2 to 0 in the flag plane."""
    seq, meta, cases, steps = hand
    row, (inner, outer) = cases[name]
    assert sorted((abs(inner - L), abs(outer - L))) == [2, 8]
    truth = seq[cases['truth'][0]]
    p1, c1, f1, _ = _row(steps, 1, row)
    p2, c2, f2, _ = _row(steps, 2, row)
    p3, c3, f3, ran3 = _row(steps, 3, row)
    p8, c8, f8, ran8 = _row(steps, 8, row)
    assert (c1, c2, c3, c8) == (1, 2, 2, 2)
    assert p1[inner] == truth[inner] and p1[outer] == seq[row, outer] != truth[outer]
    assert np.array_equal(p2, truth) and not np.array_equal(p1, p2)     # the case needs its second pass
    assert np.array_equal(p3, p2) and np.array_equal(p8, p2)
    between = range(min(inner, outer) + 1, max(inner, outer))
    assert all(f1[i] == 2 for i in between) and all(f2[i] == 0 for i in between)
    assert f1[inner] == 1 and f1[outer] == 2 and f2[inner] == f2[outer] == 1
    assert f2 != f3 and 2 in f2 and 2 not in f3          # pass 2 still leaves the two outermost bases unresolved; pass 3 trusts them
    assert f3 == f8 and sum(f3) == 2
    assert ran3 == ran8 == 3                             # pass 3 changed nothing: the row ended there


@pytest.mark.parametrize('name', ('three_pass', 'three_pass_end'))
def test_three_pass_chain(hand, name):
    seq, meta, cases, steps = hand
    row, order = cases[name]
    planes = [_row(steps, P, row)[0] for P in (1, 2, 3, 4, 8)]
    assert [_row(steps, P, row)[1] for P in (1, 2, 3, 4, 8)] == [1, 2, 3, 3, 3]
    for p, base in enumerate(order):                     # order[p] is corrected in pass p + 1, not before
        for q, plane in enumerate(planes[:3]):
            assert (plane[base] != seq[row, base]) == (q >= p)
    assert not np.array_equal(planes[0], planes[1]) and not np.array_equal(planes[1], planes[2])
    assert np.array_equal(planes[2], planes[3]) and np.array_equal(planes[2], planes[4])
    assert _row(steps, 3, row)[2] != _row(steps, 4, row)[2]             # the last 2s go in the pass that finds the fixed point
    assert _row(steps, 8, row)[3] == 4


def test_one_pass_control(hand):
    seq, meta, cases, steps = hand
    row, (base,) = cases['one_pass']
    first = _row(steps, 1, row)
    for P in (2, 3, 8):
        got = _row(steps, P, row)
        assert np.array_equal(got[0], first[0]) and got[1:3] == first[1:3] and got[3] == 2
    assert first[1] == 1 and first[2] == [0] * base + [1] + [0] * (PM.HAND_LEN - base - 1)


def test_reads_shorter_than_k_never_change():
    seq, meta, _ = PM.hand_rows(pitch=16, cut=PM.HAND_K - 1)
    plane, changed, flags, ran = PM.passes(seq, meta, PM.HAND_K, PM.HAND_T, 8)
    assert np.array_equal(plane, seq) and not changed.any() and not flags.any() and (ran == 1).all()


def test_an_n_is_fixed_in_pass_2_only_after_its_neighbour_is_corrected():
    """The two-pass row with the outer error replaced by an N: every candidate window of the N holds the inner error in pass 1."""
    seq, meta, cases = PM.hand_rows()
    row, (inner, outer) = cases['two_pass']
    truth = seq[cases['truth'][0]].copy()
    seq = seq.copy()
    seq[row, outer] = PM.NCH
    steps = PM.trace(seq, meta, PM.HAND_K, PM.HAND_T, 3, fix_n=True)
    assert steps[0][0][row, outer] == PM.NCH and steps[0][0][row, inner] == truth[inner]
    assert steps[1][0][row, outer] == truth[outer] and np.array_equal(steps[1][0][row], truth)
    assert steps[1][1][row] == 2 and steps[1][2][row, outer] == 1
    without = PM.passes(seq, meta, PM.HAND_K, PM.HAND_T, 3)
    assert without[0][row, outer] == PM.NCH and without[1][row] == 1


# ---------------------------------------------------------------- command line
def _no_ranks(monkeypatch):
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the commands then leave the memory back end alone


def test_correct_passes_reaches_main_correct_only_when_given(monkeypatch):
    from kbbq import kmer, main
    _no_ranks(monkeypatch)
    seen = []
    monkeypatch.setattr(kmer, 'main_correct', lambda path, **kw: seen.append(kw))
    main.main(['correct', '-f', 'x.fq'])
    main.main(['correct', '-f', 'x.fq', '--passes', '1'])
    main.main(['correct', '-f', 'x.fq', '--passes', '3', '--fix-n'])
    assert ['passes' in kw for kw in seen] == [False, True, True]
    assert seen[0] == dict(output=None, k=31, min_count=None, slots=None, local_slots=None, prefilter=False, filter_bits=4, fix_n=False)
    assert seen[1] == dict(seen[0], passes=1) and seen[2] == dict(seen[0], passes=3, fix_n=True)


def test_correct_summary_line(monkeypatch, capsys):
    from kbbq import kmer
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    got = []

    def fake(path, out, **kw):
        got.append(kw)
        return dict(k=kw['k'], min_count=4, reads=9, changed=np.array([1, 2]), admitted=5, slots=32)
    monkeypatch.setattr(kmer, 'correct_fastq', fake)
    kmer.main_correct('x.fq')
    kmer.main_correct('x.fq', passes=1)
    kmer.main_correct('x.fq', passes=3)
    kmer.main_correct('x.fq', passes=3, fix_n=True, prefilter=True)
    assert [kw.get('passes') for kw in got] == [None, None, 3, 3]        # passes = 1 takes exactly the call without it
    assert capsys.readouterr().err.splitlines() == [
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 passes=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 fix_n=1 passes=3 prefilter=1 admitted=5 slots=32']


@pytest.mark.parametrize('bad', (0, 9, -1, 2.5, True, '2'))
def test_python_refuses_passes_outside_1_to_8_before_any_device_call(monkeypatch, bad):
    from kbbq import _native, benchmark, kmer, recalibrate
    from kbbq.gatk import bqsr

    def never(*a, **kw):
        raise AssertionError('a device call')
    monkeypatch.setattr(_native, 'load', never)
    monkeypatch.setattr(kmer, '_ranks', never)           # ... and before anything asks for the process group
    plane, meta = np.zeros((1, 16), dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    for call in (lambda: kmer.correct_with(None, plane, meta, 2, passes=bad),
                 lambda: kmer.flag_errors(None, plane, meta, 2, passes=bad),
                 lambda: kmer.correct_batch(None, None, 2, passes=bad),
                 lambda: kmer.correct_reads(plane, meta, passes=bad),
                 lambda: kmer.correct_fastq('x.fq', 'y.fq', passes=bad),
                 lambda: kmer.correct_fastq_ranks('x.fq', 'y.fq', passes=bad),
                 lambda: kmer.main_correct('x.fq', passes=bad),
                 lambda: recalibrate.recalibrate_corrected('x.fq', passes=bad),
                 lambda: bqsr.bam_to_kmer_covariates(None, passes=bad),
                 lambda: benchmark.benchmark_kmers(None, None, None, passes=bad)):
        with pytest.raises(ValueError, match=r'passes must be an integer in 1\.\.8'):
            call()


def test_recalibrate_passes(monkeypatch, capsys):
    from kbbq import main, recalibrate as recal
    _no_ranks(monkeypatch)
    seen = []
    monkeypatch.setattr(recal, 'check_corrected', lambda *a, **kw: None)

    def fake(path, **kw):
        seen.append(kw)
        return dict(k=kw['k'], min_count=3, reads=5, changed_bases=7, admitted=11, slots=16)
    monkeypatch.setattr(recal, 'recalibrate_corrected', fake)
    main.main(['recalibrate', '-c', 'x.fq'])
    main.main(['recalibrate', '-c', 'x.fq', '--passes', '1'])
    main.main(['recalibrate', '-c', 'x.fq', '--passes', '3'])
    main.main(['recalibrate', '-c', 'x.fq', '--passes', '3', '--fix-n', '--prefilter'])
    assert [kw.get('passes') for kw in seen] == [None, 1, 3, 3]         # without the option: the call as it was
    assert seen[0] == dict(infer_rg=False, gatkreport=None, output=None, k=31, min_count=None, slots=None, prefilter=False,
                           filter_bits=4)
    lines = [x for x in capsys.readouterr().err.splitlines() if x.startswith('kbbq recalibrate:')]
    assert lines == ['kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 passes=3',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 fix_n=1 passes=3 prefilter=1 admitted=11 slots=16']


@pytest.mark.parametrize('argv', (['recalibrate', '-f', 'a.fq', 'b.fq', '--passes', '2'], ['recalibrate', '-b', 'a.bam', '--passes', '2']))
def test_recalibrate_passes_only_with_correct(monkeypatch, capsys, argv):
    from kbbq import main, recalibrate as recal
    _no_ranks(monkeypatch)
    monkeypatch.setattr(recal, 'recalibrate', lambda **kw: pytest.fail('ran'))
    with pytest.raises(SystemExit) as exc:
        main.main(argv)
    assert exc.value.code == 2
    assert '--passes: only with -c/--correct' in capsys.readouterr().err


class _Report:
    def write(self, path):
        pass


def _bqsr_patched(monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    _no_ranks(monkeypatch)
    seen = []

    def kmers(bam, **kw):
        seen.append(kw)
        kw['info'].update(k=kw['k'], min_count=7, reads=5, flagged_bases=11, admitted=13, slots=1024)
        if kw.get('skip_unresolved'):
            kw['info'].update(skipped_bases=17)
        return _Report()
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: 'opened:' + p)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', kmers)
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: pytest.fail('the reference path ran'))
    return seen


def test_bqsr_passes(monkeypatch, capsys):
    from kbbq import main
    seen = _bqsr_patched(monkeypatch)
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp'])
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp', '--passes', '1'])
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp', '--passes', '3'])
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp', '--passes', '3', '--skip-unresolved', '--prefilter'])
    for kw in seen:
        kw.pop('info')
    assert seen[0] == dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, use_oq=False)
    assert seen[1] == dict(seen[0], passes=1) and seen[2] == dict(seen[0], passes=3)
    assert seen[3] == dict(seen[0], passes=3, skip_unresolved=True, prefilter=True)
    assert capsys.readouterr().err.splitlines() == [
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11',
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11',
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11 passes=3',
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11 skipped_bases=17 passes=3 prefilter=1 admitted=13 slots=1024']


def test_bqsr_passes_only_with_kmers(monkeypatch, capsys):
    from kbbq import main
    seen = _bqsr_patched(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--passes', '2'])
    assert exc.value.code == 2 and not seen
    assert '--passes: only with --kmers' in capsys.readouterr().err


def test_the_keyword_reaches_the_covariates_only_when_it_is_not_1(monkeypatch):
    from kbbq.gatk import bqsr
    seen = {}
    monkeypatch.setattr(bqsr.utils, 'get_rg_to_pu', lambda bam: {'g0': 'unit0'})
    monkeypatch.setattr(bqsr, 'bam_to_kmer_covariates', lambda bam, **kw: seen.update(kw=kw) or 'vectors')
    monkeypatch.setattr(bqsr, 'vectors_to_report', lambda *a: a)
    bqsr.bam_to_report_kmers('bam', k=15, passes=2)
    assert seen['kw']['passes'] == 2
    bqsr.bam_to_report_kmers('bam', k=15)
    assert 'passes' not in seen['kw']


def test_benchmark_passes(monkeypatch, capsys):
    from kbbq import benchmark as bm, main
    _no_ranks(monkeypatch)
    seen = []
    monkeypatch.setattr(bm, 'benchmark', lambda **kw: seen.append(kw))
    base = ['benchmark', '-b', 'x.sam', '-r', 'x.fa', '-v', 'x.vcf', '--kmers']
    main.main(base)
    main.main(base + ['--passes', '1'])
    main.main(base + ['--passes', '3'])
    plain = dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4)
    assert [kw['kmers'] for kw in seen] == [plain, dict(plain, passes=1), dict(plain, passes=3)]
    with pytest.raises(SystemExit) as exc:
        main.main(base[:-1] + ['--passes', '2'])
    assert exc.value.code == 2 and len(seen) == 3
    assert '--passes: only with --kmers' in capsys.readouterr().err


def test_benchmark_summary_line():
    from kbbq import benchmark as bm
    info = dict(k=31, min_count=4, reads=9, bases=100, errors=10, flagged=8, flagged_errors=8, unresolved=5, unresolved_errors=1,
                prefilter=False, admitted=None, slots=64)
    line = ('kbbq benchmark: k=31 min_count=4 reads=9 bases=100 errors=10 flagged=8 flagged_errors=8 unresolved=5 '
            'unresolved_errors=1 precision=1.0000 recall=0.8000')
    assert bm.kmer_summary(info) == bm.kmer_summary(dict(info, passes=1)) == line
    assert bm.kmer_summary(dict(info, passes=3)) == line + ' passes=3'
    assert bm.kmer_summary(dict(info, passes=3, prefilter=True, admitted=7)) == line + ' passes=3 prefilter=1 admitted=7 slots=64'


@pytest.mark.parametrize('command', (['correct', '-f', 'x.fq'], ['recalibrate', '-c', 'x.fq'], ['bqsr', '-b', 'x', '--kmers', '-g', 'r'],
                                     ['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '--kmers']))
@pytest.mark.parametrize('value', ('0', '9', 'two'))
def test_values_outside_1_to_8_are_argparse_errors(monkeypatch, capsys, command, value):
    from kbbq import main
    _no_ranks(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(command + ['--passes', value])
    assert exc.value.code == 2
    assert 'argument --passes' in capsys.readouterr().err


# ---------------------------------------------------------------- the C ABI
SIBLINGS = {'kbbq_kmer_correct_passes_dev': 'kbbq_kmer_correct_ex_dev', 'kbbq_kmer_correct_passes': 'kbbq_kmer_correct_ex',
            'kbbq_kmer_correct_rows_passes_dev': 'kbbq_kmer_correct_rows_ex_dev', 'kbbq_kmer_flag_passes_dev': 'kbbq_kmer_flag_ex_dev'}


def test_symbols_are_exported_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    for name, sibling in SIBLINGS.items():
        assert hasattr(lib, name)
        ret, args = N.PROTOTYPES[sibling]
        assert N.PROTOTYPES[name] == (ret, args + [ret])                # the sibling's arguments and `int passes`
        assert re.search(r'^int %s\(kbbq_ctx\* ctx, const kbbq_kmer_table\* table,' % name, header, flags=re.M)
    assert N.KMER_MAX_PASSES == 8


def test_device_free_refusals_of_the_calls():
    """No context and no table exist without a device: every refusal below is decided on the arguments alone."""
    from kbbq import _native as N
    lib = N.load()
    calls = {
        'kbbq_kmer_correct_passes_dev': lambda n, pitch, t, opts, P: lib.kbbq_kmer_correct_passes_dev(None, None, None, None, n, pitch, t, None, None, opts, P),
        'kbbq_kmer_correct_passes': lambda n, pitch, t, opts, P: lib.kbbq_kmer_correct_passes(None, None, None, None, n, pitch, t, None, None, opts, P),
        'kbbq_kmer_correct_rows_passes_dev': lambda n, pitch, t, opts, P: lib.kbbq_kmer_correct_rows_passes_dev(None, None, None, None, n, pitch, 0, t, None, None, opts, P),
        'kbbq_kmer_flag_passes_dev': lambda n, pitch, t, opts, P: lib.kbbq_kmer_flag_passes_dev(None, None, None, None, n, pitch, t, None, None, None, opts, P),
    }
    for name, call in calls.items():
        for P in (0, 9, -1, 1 << 20):                    # before anything else, whatever the other arguments are
            assert call(1, 17, 0, 0x100, P) == N.KBBQ_E_ARG
            assert name in N.last_error() and 'passes must be in 1..8' in N.last_error()
        for P in (1, 2, 8):                              # the sibling's refusals stay
            assert call(0, 16, 2, 0x100, P) == N.KBBQ_E_ARG
            assert name in N.last_error() and 'opts' in N.last_error()
            assert call(0, 16, 2, 0, P) == N.KBBQ_E_ARG
            assert 'NULL ctx or table' in N.last_error()
    flag = calls['kbbq_kmer_flag_passes_dev']
    assert flag(0, 16, 2, N.KMER_FIX_N, 2) == N.KBBQ_E_ARG and 'no N rule' in N.last_error()
    assert flag(1, 17, 2, N.KMER_FLAG_UNRESOLVED, 2) == N.KBBQ_E_ARG and 'pitch must be a positive multiple of 16' in N.last_error()
    assert flag(1, 16, 0, N.KMER_FLAG_UNRESOLVED, 2) == N.KBBQ_E_ARG and 'min_count must be >= 1' in N.last_error()
