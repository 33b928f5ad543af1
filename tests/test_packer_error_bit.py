"""KBBQ_ROWS_ERRBIT on the host (include/kbbq_hip.h): kbbq_fastq_fill_rows with the flag against a NumPy statement of the
nibbles -- bits 0-2 the code, bit 3 "the corrected read's code differs" --, the corrected plane left unwritten when no
destination is given, and the entry points that refuse the flag.  The GPU twin is tests/test_gpu_layout_error_bit.py."""
import ctypes

import numpy as np
import pytest

from kbbq import _native as N
from kbbq import fastx
from test_packer_layouts import _pair_files, np_layout

EB = N.ROWS_PAIRS | N.ROWS_NIBBLES | N.ROWS_ERRBIT


def np_error_bit(seq_nib, cseq_nib):
    """The seq plane of an ERRBIT layout from the two 4-bit planes of the same rows."""
    x = seq_nib ^ cseq_nib
    return seq_nib | np.where(x & 0x0F, 0x08, 0).astype(np.uint8) | np.where(x & 0xF0, 0x80, 0).astype(np.uint8)


@pytest.mark.parametrize('n,S,nrg,single_end', [(40, 150, 1, False), (66, 100, 3, False), (33, 150, 1, True), (2, 150, 1, False)])
def test_fill_rows_sets_bit_3_where_the_corrected_read_differs(tmp_path, n, S, nrg, single_end):
    rng = np.random.default_rng(n * 1000 + S)
    fa, fb = _pair_files(tmp_path, rng, n, S, nrg, single_end)
    infer = nrg > 1
    A, B, info = fastx.PairScan(fa, fb, infer).result()
    R = info[2]
    pitch = fastx.pitch_for(S)
    seq, cseq, qual, meta = A.fill(B, infer, n, pitch)
    assert (seq != cseq).any()
    flags = EB | (N.ROWS_TWINS if single_end else 0)
    nrows = (n + 1) // 2
    perm = None
    if R > 1:
        perm, seg = np.empty(nrows, dtype=np.int64), np.empty(R + 1, dtype=np.int64)
        N.check(N.load().kbbq_group_rows_host(N.ptr(meta), nrows, 1, R, N.ptr(perm), N.ptr(seg)))
    wseq, wcseq, wqual, wmeta = np_layout(seq, cseq, qual, meta, flags & ~N.ROWS_ERRBIT, S, perm)
    want = np_error_bit(wseq, wcseq)
    assert (want & 0x88).any() and ((want & 0x77) == wseq).all()
    dp = wqual.shape[1]
    sp = dp // 2
    assert dp // 16 in (19, 13)
    # separator and padding: code 4, bit 3 clear -- base S (and everything from 2S + 1 on) of every row
    for base in [S] + list(range(2 * S + 1, dp)):
        byte, high = (base // 16) * 8 + (base % 16) % 4 + 4 * ((base % 16) // 8), (base % 8) >= 4
        assert ((want[:, byte] >> (4 if high else 0)) & 0x0F == 4).all()
    got = [np.zeros((nrows, sp), np.uint8), np.zeros((nrows, sp), np.uint8), np.zeros((nrows, dp), np.uint8), np.zeros(nrows, np.uint32)]
    cut = nrows // 3
    for lo, m in ((0, cut), (cut, nrows - cut)):
        assert not A.fill_rows(B, 0, n, meta, flags, 2 * S, dp, perm, lo, m, got[0][lo:lo + m], got[1][lo:lo + m], got[2][lo:lo + m], got[3][lo:lo + m])
    for g, w, name in zip(got, (want, wcseq, wqual, wmeta), ('seq', 'cseq', 'qual', 'meta')):
        assert np.array_equal(g, w), name
    # no destination for the corrected plane: the same seq / qual / meta, nothing else written
    only = [np.zeros((nrows, sp), np.uint8), np.zeros((nrows, dp), np.uint8), np.zeros(nrows, np.uint32)]
    assert not A.fill_rows(B, 0, n, meta, flags, 2 * S, dp, perm, 0, nrows, only[0], None, only[1], only[2])
    assert np.array_equal(only[0], want) and np.array_equal(only[1], wqual) and np.array_equal(only[2], wmeta)


def test_fill_rows_refuses_the_flag_where_it_has_no_meaning(tmp_path):
    rng = np.random.default_rng(5)
    fa, fb = _pair_files(tmp_path, rng, 20, 150, 1)
    A, B, info = fastx.PairScan(fa, fb, False).result()
    meta, st = A.meta(False, 0, 20)
    dp = 304
    bufs = lambda: (np.zeros((10, dp // 2), np.uint8), np.zeros((10, dp // 2), np.uint8), np.zeros((10, dp), np.uint8), np.zeros(10, np.uint32))
    for flags, other, S2 in ((EB, None, 300),                                   # no corrected reads to compare with
                             (N.ROWS_PAIRS | N.ROWS_ERRBIT, B, 300),            # character planes
                             (N.ROWS_NIBBLES | N.ROWS_ERRBIT, B, 300),          # one read per row
                             (EB, B, 150)):                                     # rows of 10 chunks: no kernel instance reads them
        with pytest.raises(ValueError, match='kbbq_fastq_fill_rows'):       # KBBQ_E_ARG, naming the call
            A.fill_rows(other, 0, 20, meta, flags, S2, dp, None, 0, 10, *bufs())
        s, c, q, m = bufs()
        lib = N.load()
        rc = lib.kbbq_fastq_fill_rows(A._h, other._h if other is not None else None, 0, 20, N.ptr(meta), flags, S2, dp, None, 0, 10,
                                      N.ptr(s), N.ptr(c), N.ptr(q), N.ptr(m), ctypes.byref(ctypes.c_int(0)))
        assert rc == N.KBBQ_E_ARG
    # a character outside ACGTN in the corrected read is still reported (the caller drops NIBBLES and ERRBIT together)
    text = open(fb).read().split('\n')
    text[1] = 'a' + text[1][1:]
    open(fb, 'w').write('\n'.join(text))
    A, B, info = fastx.PairScan(fa, fb, False).result()
    assert A.fill_rows(B, 0, 20, meta, EB, 300, dp, None, 0, 10, *bufs())


def test_the_calls_that_would_read_bit_3_as_code_refuse_the_flag():
    """The k-mer calls on rows check their KBBQ_ROWS_* flags before they look at any other argument (no device is needed
    to be refused): KBBQ_E_ARG, the message names the call and the flag.  Without the flag the same calls get as far as
    their NULL context."""
    lib = N.load()
    calls = {'kbbq_kmer_count_rows_dev': lambda f: lib.kbbq_kmer_count_rows_dev(None, None, None, None, 0, 304, f),
             'kbbq_kmer_prefilter_rows_dev': lambda f: lib.kbbq_kmer_prefilter_rows_dev(None, None, 31, None, None, 0, 304, f),
             'kbbq_kmer_count_filtered_rows_dev': lambda f: lib.kbbq_kmer_count_filtered_rows_dev(None, None, None, None, None, 0, 304, f)}
    for name, call in calls.items():
        assert call(EB) == N.KBBQ_E_ARG
        msg = lib.kbbq_last_error().decode()
        assert name in msg and 'KBBQ_ROWS_ERRBIT' in msg
        assert call(EB & ~N.ROWS_ERRBIT) == N.KBBQ_E_ARG and 'KBBQ_ROWS_ERRBIT' not in lib.kbbq_last_error().decode()


def test_layout_choice_in_python():
    """errbit_flag: where lay_out / laid_from_reader set the flag by default, where they cannot, and the refusal."""
    from kbbq import _device as dev
    two = N.ROWS_PAIRS | N.ROWS_NIBBLES
    assert dev.errbit_flag(two, 150, True) == N.ROWS_ERRBIT and dev.errbit_flag(two | N.ROWS_TWINS, 100, True) == N.ROWS_ERRBIT
    assert dev.errbit_flag(two, 150, True, errbit=False) == 0
    assert dev.errbit_flag(two, 150, False) == 0                        # no corrected reads
    assert dev.errbit_flag(two, 50, True) == 0                          # 7 chunks
    assert dev.errbit_flag(N.ROWS_PAIRS, 150, True) == 0 and dev.errbit_flag(N.ROWS_NIBBLES, 150, True) == 0
    with pytest.raises(ValueError):
        dev.errbit_flag(N.ROWS_NIBBLES, 150, True, errbit=True)
    b = dev.PairBatch.__new__(dev.PairBatch)
    b.nib, b.twins, b.errbit = True, False, True
    assert dev._row_flags(b) == two | N.ROWS_ERRBIT and b.layout_key() == 'pairs_nib'
