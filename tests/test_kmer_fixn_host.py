"""kbbq correct --fix-n without a GPU: the CPU model of the N rule (tests/kmer_fixn_model.py) on a hand-worked example and
against kmer_model with the rule off, the command line's new flag, the new symbols of the C ABI and their refusal of unknown
option bits, and the N-carrying read set the GPU tests compare on."""
import ctypes
import os
import re

import numpy as np
import pytest

import kmer_fixn_model as F
import kmer_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = ('kbbq_kmer_correct_ex_dev', 'kbbq_kmer_correct_ex', 'kbbq_kmer_correct_rows_ex_dev')


def test_six_reads_worked_by_hand():
    """k = 8, t = 2.  R twice and its variant V (base 7 T -> C) twice make every 8-mer of both solid.
    Read 5, R with an N at 7: its 8 candidate windows are solid with T (R) and with C (V) alike -- a tie, it stays N.
    Read 6, R with Ns at 12 and 14: the windows over 12 that miss 14 are [5, 13) and [6, 14), solid with A alone (R's 8-mers;
    V has C at 7), so 12 becomes A; both windows over 14, [7, 15) and [8, 16), hold 12 as well: no candidate, it stays N."""
    R = b'ACGGTCATTGCAAGCT'
    V = b'ACGGTCACTGCAAGCT'
    reads = [R, R, V, V, b'ACGGTCANTGCAAGCT', b'ACGGTCATTGCANGNT']
    seq, meta = M.plane(reads)
    out, changed, t, kinds = F.correct(seq, meta, 8, 2)
    assert [out[i, :16].tobytes() for i in range(6)] == [R, R, V, V, b'ACGGTCANTGCAAGCT', b'ACGGTCATTGCAAGNT']
    assert changed.tolist() == [0, 0, 0, 0, 0, 1] and t == 2
    assert kinds == {(4, 7): 'tie', (5, 12): 'fixed', (5, 14): 'second_break'}
    # a separator is no N: with base 7 of read 5 named as one, nothing looks at it
    sep = [None, None, None, None, 7, None]
    assert (4, 7) not in F.correct(seq, meta, 8, 2, sep=sep)[3]
    # only the character N: a lower-case n is a break that stays
    seq2 = seq.copy()
    seq2[5, 12] = ord('n')
    out2, changed2, _, kinds2 = F.correct(seq2, meta, 8, 2)
    assert out2[5, :16].tobytes() == b'ACGGTCATTGCAnGNT' and changed2.sum() == 0 and (5, 12) not in kinds2


@pytest.fixture(scope='module')
def reads15():
    return F.with_ns(7, 15)


def test_the_rule_off_is_kmer_model(reads15):
    seq, meta, _ = reads15
    want, want_changed, wt = M.correct(seq, meta, 15)
    out, changed, t, kinds = F.correct(seq, meta, 15, fix_n=False)
    assert t == wt and kinds == {} and np.array_equal(out, want) and np.array_equal(changed, want_changed)
    # ... and with it on, the bases that are not N are decided as without it
    on, on_changed, _, kinds = F.correct(seq, meta, 15)
    fixed = np.zeros(seq.shape, dtype=bool)
    for (r, i), kind in kinds.items():
        fixed[r, i] = kind == 'fixed'
    assert np.array_equal(on[~fixed], want[~fixed]) and np.all(seq[fixed] == ord('N')) and np.all(on[fixed] != ord('N'))
    assert np.array_equal(on_changed - want_changed, fixed.sum(axis=1))
    rng = np.random.default_rng(0)
    for k in (8, 15, 31, 32):
        for f in rng.integers(0, 1 << 62, 50).tolist():
            f &= (1 << (2 * k)) - 1
            assert F.revcomp(f, k) == M.revcomp(f, k)


@pytest.mark.parametrize('k', [15, 32])
def test_the_read_set_has_an_n_of_each_kind(reads15, k):
    seq, meta, cases = reads15 if k == 15 else F.with_ns(7, k)
    out, changed, t, kinds = F.correct(seq, meta, k)
    n = F.kind_counts(kinds)
    assert n['fixed'] >= 100 and n['tie'] >= 1 and n['none'] >= 1 and n['second_break'] >= 1 and n['no_window'] >= 1
    assert sum(n.values()) == int(((seq == ord('N')) & (np.arange(seq.shape[1])[None, :] < meta.astype(np.int64)[:, None])).sum())
    for name in ('first', 'last', 'b15', 'b16', 'b31', 'b32', 'exactly_k', 'pair_d%d' % k, 'pair_d%d_second' % k):
        assert kinds[cases[name]] == 'fixed', name
    for d in (1, k - 1, k + 1):
        assert cases['pair_d%d' % d] in kinds and cases['pair_d%d_second' % d] in kinds
    assert kinds[cases['tie']] == 'tie' and kinds[cases['errors']] == 'none' and kinds[cases['shorter_than_k']] == 'no_window'
    assert cases['first'][1] == 0 and cases['last'][1] == int(meta[cases['last'][0]]) - 1
    assert int(meta[cases['exactly_k'][0]]) == k and int(meta[cases['shorter_than_k'][0]]) == k - 1
    r, i = cases['b16']
    assert out[r, i] != ord('N') and changed[r] >= 1


def test_argparse_takes_fix_n(monkeypatch, capsys):
    from kbbq import kmer, main
    from kbbq import recalibrate as recal
    calls = []
    monkeypatch.setattr(kmer, 'main_correct', lambda *a, **kw: calls.append(kw))
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the command then leaves the memory back end alone
    main.main(['correct', '-f', 'x.fq'])
    main.main(['correct', '-f', 'x.fq', '--fix-n'])
    main.main(['correct', '-f', 'x.fq', '--fix-n', '--prefilter'])
    assert [(kw['fix_n'], kw['prefilter']) for kw in calls] == [(False, False), (True, False), (True, True)]
    # recalibrate: with -c it reaches recalibrate_corrected, and the summary line says so; without -c it is refused
    seen = []
    monkeypatch.setattr(recal, 'check_corrected', lambda *a, **kw: None)

    def fake(path, **kw):
        seen.append(kw)
        return dict(k=kw['k'], min_count=3, reads=5, changed_bases=7, admitted=11, slots=16)
    monkeypatch.setattr(recal, 'recalibrate_corrected', fake)
    main.main(['recalibrate', '-c', 'x.fq'])
    main.main(['recalibrate', '-c', 'x.fq', '--fix-n'])
    main.main(['recalibrate', '-c', 'x.fq', '--fix-n', '--prefilter'])
    assert [kw.get('fix_n', False) for kw in seen] == [False, True, True]     # without the flag: the call as it was
    lines = [x for x in capsys.readouterr().err.splitlines() if x.startswith('kbbq recalibrate:')]
    assert lines == ['kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 fix_n=1',
                     'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7 fix_n=1 prefilter=1 admitted=11 slots=16']
    for argv in (['recalibrate', '-f', 'a.fq', 'b.fq', '--fix-n'], ['recalibrate', '-b', 'a.bam', '--fix-n']):
        with pytest.raises(SystemExit):
            main.main(argv)
        assert re.search(r'--fix-n: only with -c/--correct', capsys.readouterr().err)


def test_the_summary_line_of_correct(monkeypatch, capsys):
    from kbbq import kmer
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    got = []

    def fake(path, out, **kw):
        got.append(kw)
        return dict(k=kw['k'], min_count=4, reads=9, changed=np.array([1, 2]), admitted=5, slots=32)
    monkeypatch.setattr(kmer, 'correct_fastq', fake)
    kmer.main_correct('x.fq')
    kmer.main_correct('x.fq', fix_n=True)
    kmer.main_correct('x.fq', fix_n=True, prefilter=True)
    assert [kw['fix_n'] for kw in got] == [False, True, True]
    assert capsys.readouterr().err.splitlines() == [
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 fix_n=1',
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3 fix_n=1 prefilter=1 admitted=5 slots=32']


def test_the_new_symbols_are_declared_and_exported():
    from kbbq import _native as N
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    assert re.search(r'^#define KBBQ_KMER_FIX_N 1$', header, flags=re.M) and N.KMER_FIX_N == 1
    lib = N.load()
    assert re.search(r'^#define KBBQ_ABI_VERSION 1$', header, flags=re.M) and lib.kbbq_abi_version() == 1
    for name in EX:
        assert re.search(r'^int %s\(kbbq_ctx\* ctx, .*int opts\);' % name, header, flags=re.M | re.S), name
        # the counterpart's arguments plus one int
        assert getattr(lib, name).argtypes[:-1] == getattr(lib, name.replace('_ex', '')).argtypes
        assert getattr(lib, name).argtypes[-1] is ctypes.c_int


def test_unknown_option_bits_are_refused_without_a_device():
    from kbbq import _native as N
    lib = N.load()
    for opts in (2, 3, 4, 1 << 16, -2):
        for name in EX:
            rows = (0,) if 'rows' in name else ()            # the KBBQ_ROWS_* word, valid: it is `opts` that is refused
            rc = getattr(lib, name)(None, None, None, None, 0, 16, *rows, 2, None, None, opts)
            assert rc == N.KBBQ_E_ARG
            assert 'opts' in N.last_error() and name in N.last_error()
    # a known word gets past that check: what is refused then is the missing context
    for name in EX:
        rows = (0,) if 'rows' in name else ()
        for opts in (0, N.KMER_FIX_N):
            assert getattr(lib, name)(None, None, None, None, 0, 16, *rows, 2, None, None, opts) == N.KBBQ_E_ARG
            assert 'opts' not in N.last_error() and 'NULL' in N.last_error()
