"""`kbbq recalibrate -c --skip-unresolved`, host side, no GPU: the flag on the command line, the keyword main passes only when
the flag is given, the new entry point in the header, in kbbq._native.PROTOTYPES and in the built library, and the construction
the GPU test's expectation rests on -- a low quality at base i takes base i, and base i alone, out of the dinucleotide contexts."""
import ctypes
import os
import re

import numpy as np
import pytest

from kmer_skip_model import masked_quals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_vp, _i, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
NAME = 'kbbq_kmer_correct_rows_skip_dev'
# ctx, table, d_seq, d_meta, nrows, pitch, flags, min_count, d_out, d_changed, opts, passes, d_qual, d_tally_qual, d_unresolved
ARGS = [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]


def _header_types(name):
    """ctypes of the parameters of `name` as include/kbbq_hip.h declares it: pointers, int64_t, int."""
    with open(os.path.join(ROOT, 'include', 'kbbq_hip.h')) as fh:
        text = fh.read()
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, text, re.S)
    assert m, '%s is not declared in the header' % name
    out = []
    for param in m.group(1).split(','):
        param = ' '.join(param.split())
        out.append(_vp if '*' in param else _i64 if param.startswith('int64_t') else _i if param.startswith('int ') else None)
    return out


def test_the_call_is_declared_bound_and_exported():
    from kbbq import _native as N
    assert _header_types(NAME) == ARGS
    res, args = N.PROTOTYPES[NAME]
    assert res is _i and args == ARGS
    fn = getattr(N.load(), NAME)                             # AttributeError when the library lacks it
    assert fn.restype is _i and list(fn.argtypes) == ARGS
    assert N.load().kbbq_abi_version() == 1
    with open(os.path.join(ROOT, 'include', 'kbbq_hip.h')) as fh:
        text = fh.read()
    assert text.index('"Row readers"') < text.index(NAME + ' (')      # documented with the calls on resident rows


def test_bad_arguments_are_refused_without_a_device():
    from kbbq import _native as N
    lib = N.load()
    q, t = ctypes.c_void_p(4096), ctypes.c_void_p(8192)

    def call(opts=0, passes=1, flags=0, d_qual=q, d_tally=t):
        return lib.kbbq_kmer_correct_rows_skip_dev(None, None, None, None, 0, 16, flags, 2, None, None, opts, passes, d_qual, d_tally, None)
    for kw, word in ((dict(opts=N.KMER_FLAG_UNRESOLVED), 'opts'), (dict(opts=4), 'opts'), (dict(opts=N.KMER_FIX_N | 2), 'opts'),
                     (dict(passes=0), 'passes'), (dict(passes=9), 'passes'), (dict(flags=8), 'flags'), (dict(flags=N.ROWS_TWINS), 'TWINS'),
                     (dict(d_qual=None), 'd_qual'), (dict(d_tally=None), 'd_tally_qual'), (dict(d_tally=q), 'd_tally_qual is d_qual'),
                     (dict(d_tally=ctypes.c_void_p(8200)), 'aligned'),
                     (dict(), 'NULL ctx or table')):
        assert call(**kw) == N.KBBQ_E_ARG, kw
        assert word in N.last_error(), (kw, N.last_error())


@pytest.fixture
def cli(monkeypatch):
    """main.main with both recalibrate paths recorded instead of run."""
    from kbbq import main, recalibrate
    calls = []
    monkeypatch.setattr(recalibrate, 'recalibrate', lambda **kw: calls.append(('two', kw)))
    monkeypatch.setattr(recalibrate, 'recalibrate_corrected',
                        lambda path, **kw: calls.append(('one', dict(kw, path=path))) or
                        dict(k=kw['k'], min_count=4, reads=10, changed_bases=7, slots=2048, admitted=99, skipped_bases=5))
    monkeypatch.setattr(recalibrate, 'check_corrected', lambda *a, **kw: None)
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                # the command then leaves the memory back end alone
    return main, calls


def test_main_passes_the_keyword_only_when_the_flag_is_given(cli, capsys):
    main, calls = cli
    main.main(['recalibrate', '-c', 'x.fq'])
    assert calls[0] == ('one', dict(path='x.fq', infer_rg=False, gatkreport=None, output=None, k=31, min_count=None, slots=None,
                                    prefilter=False, filter_bits=4))
    assert capsys.readouterr().err == 'kbbq recalibrate: k=31 min_count=4 reads=10 changed_bases=7\n'
    main.main(['recalibrate', '-c', 'x.fq', '--skip-unresolved'])
    assert calls[1] == ('one', dict(path='x.fq', infer_rg=False, gatkreport=None, output=None, k=31, min_count=None, slots=None,
                                    prefilter=False, filter_bits=4, skip_unresolved=True))
    assert capsys.readouterr().err == 'kbbq recalibrate: k=31 min_count=4 reads=10 changed_bases=7 skipped_bases=5\n'
    main.main(['recalibrate', '-c', 'x.fq', '--skip-unresolved', '--fix-n', '--passes', '3', '--prefilter', '--infer-rg', '-g', 'm.txt'])
    assert calls[2] == ('one', dict(path='x.fq', infer_rg=True, gatkreport='m.txt', output=None, k=31, min_count=None, slots=None,
                                    prefilter=True, filter_bits=4, fix_n=True, passes=3, skip_unresolved=True))
    assert capsys.readouterr().err == ('kbbq recalibrate: k=31 min_count=4 reads=10 changed_bases=7 skipped_bases=5 fix_n=1 passes=3 '
                                       'prefilter=1 admitted=99 slots=2048\n')


@pytest.mark.parametrize('argv', (['-f', 'a.fq', 'b.fq', '--skip-unresolved'], ['-b', 'x.bam', '--skip-unresolved']))
def test_the_flag_without_c_is_an_error_that_names_it(cli, argv, capsys):
    main, calls = cli
    with pytest.raises(SystemExit) as e:
        main.main(['recalibrate'] + argv)
    assert e.value.code == 2 and not calls
    err = capsys.readouterr().err
    assert '--skip-unresolved: only with -c/--correct' in err


def test_the_keyword_reaches_the_refusals_and_the_signature(monkeypatch):
    """recalibrate_corrected and correct_batch take the keyword, default off; what -c refuses it refuses with it, before any device
    call."""
    import inspect
    from kbbq import kmer, recalibrate
    assert inspect.signature(recalibrate.recalibrate_corrected).parameters['skip_unresolved'].default is False
    assert inspect.signature(kmer.correct_batch).parameters['skip_unresolved'].default is False
    monkeypatch.setattr(kmer, '_ranks', lambda: (2, 1))
    with pytest.raises(ValueError, match='ranks'):
        recalibrate.recalibrate_corrected('reads.fq', skip_unresolved=True)


def test_a_low_quality_at_base_i_changes_the_context_of_base_i_alone():
    """The masked file of the GPU test (tests/kmer_skip_model.py) against generic_dinuc_covariate on one hand-made read: the
    contexts of the class-2 bases become -1, every other context is what it was -- the base after a masked one included, whose
    context still names the masked base's letter."""
    from kbbq import compare_reads
    read = 'ACGTTGCANACGGTCA'
    seq = np.array(list(read), dtype='U1')
    qual = np.array([30, 7, 6, 5, 40, 40, 12, 9, 30, 30, 2, 41, 20, 20, 6, 33], dtype=np.uint8) + 33
    cls = np.zeros(len(read), dtype=np.uint8)
    cls[[0, 2, 5, 6, 9, 15]] = 2                             # the first base, neighbours of each other, beside the N, the last base
    cls[[4, 12]] = 1                                         # a changed base is no unresolved one
    before = compare_reads.generic_dinuc_covariate(seq, qual.astype(np.int_) - 33, 6)
    for byte in (ord('!'), 0):                               # the file's character and the device plane's byte
        masked = masked_quals(qual, cls, byte)
        assert np.array_equal(masked[cls != 2], qual[cls != 2]) and (masked[cls == 2] == byte).all()
        after = compare_reads.generic_dinuc_covariate(seq, masked.astype(np.int_) - 33, 6)
        assert (after[cls == 2] == -1).all()
        assert np.array_equal(after[cls != 2], before[cls != 2])
    assert before[3] == -1 and before[10] == -1              # quality below 6: out already
    assert before[7] >= 0 and before[1] >= 0 and before[2] >= 0 and before[6] >= 0      # base 7 follows masked base 6 and keeps its context
    assert (before[[8, 9]] == -1).all()                      # the N and the base after it have none
