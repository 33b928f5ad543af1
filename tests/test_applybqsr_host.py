"""
Host-side parts of ApplyBQSR on aligned reads (no GPU): the native SAM rewriter (kbbq_sam_render), the model forms the
batch path chooses (kbbq.gatk.applybqsr._model), the two new sub-commands' arguments and the new C ABI symbols.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SAM = ('@HD\tVN:1.6\n@RG\tID:g0\tPU:u0\n@CO\tfree text\n'
       'a\t0\tc\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tOQ:Z:5555\tRG:Z:g0\n'
       'b\t16\tc\t5\t60\t3M\t*\t0\t0\tACG\t#$%\tRG:Z:g0\n'
       'c\t4\t*\t0\t0\t*\t*\t0\t0\tAC\t*\tRG:Z:g0\n'
       'd\t0\tc\t9\t60\t2M\t*\t0\t0\tTT\tAB\r\n')


def _render(bam, plane, set_oq, first=0, n=None):
    from kbbq import _native as N
    lib = N.load()
    b = bam.batch()
    n = b.n - first if n is None else n
    need = ctypes.c_size_t(0)
    N.check(lib.kbbq_sam_render(b._native, first, n, N.ptr(plane), plane.shape[1], set_oq, None, 0, ctypes.byref(need)))
    out = np.zeros(need.value + 1, dtype=np.uint8)
    N.check(lib.kbbq_sam_render(b._native, first, n, N.ptr(plane), plane.shape[1], set_oq, N.ptr(out), out.nbytes,
                                ctypes.byref(need)))
    small = np.zeros(max(need.value - 1, 1), dtype=np.uint8)
    with pytest.raises(ValueError):
        N.check(lib.kbbq_sam_render(b._native, first, n, N.ptr(plane), plane.shape[1], set_oq, N.ptr(small), small.nbytes,
                                    ctypes.byref(need)))
    return bytes(out[:need.value]).decode()


def test_sam_render_replaces_qual_and_adds_oq(tmp_path):
    from kbbq import aln
    p = tmp_path / 'in.sam'
    p.write_bytes(SAM.encode())
    bam = aln.AlignmentFile(str(p))
    plane = np.zeros((4, 16), dtype=np.uint8)
    plane[0, :4] = list(b'++++')
    plane[1, :3] = list(b'!!!')
    plane[3, :2] = list(b'77')
    got = _render(bam, plane, 0)
    assert got == ('a\t0\tc\t1\t60\t4M\t*\t0\t0\tACGT\t++++\tOQ:Z:5555\tRG:Z:g0\n'
                   'b\t16\tc\t5\t60\t3M\t*\t0\t0\tACG\t!!!\tRG:Z:g0\n'
                   'c\t4\t*\t0\t0\t*\t*\t0\t0\tAC\t*\tRG:Z:g0\n'
                   'd\t0\tc\t9\t60\t2M\t*\t0\t0\tTT\t77\n')
    got = _render(bam, plane, 1)
    assert got.splitlines() == ['a\t0\tc\t1\t60\t4M\t*\t0\t0\tACGT\t++++\tOQ:Z:5555\tRG:Z:g0',          # an OQ tag is kept
                                'b\t16\tc\t5\t60\t3M\t*\t0\t0\tACG\t!!!\tRG:Z:g0\tOQ:Z:#$%',
                                'c\t4\t*\t0\t0\t*\t*\t0\t0\tAC\t*\tRG:Z:g0',                          # '*': nothing to keep
                                'd\t0\tc\t9\t60\t2M\t*\t0\t0\tTT\t77\tOQ:Z:AB']
    assert _render(bam, plane[1:3], 1, first=1, n=2) == '\n'.join(got.splitlines()[1:3]) + '\n'
    # the header as the writer copies it
    assert list(bam.header) == ['@HD\tVN:1.6', '@RG\tID:g0\tPU:u0', '@CO\tfree text']


def test_model_forms():
    """Integer models use kbbq_build_lut's blob; a float model only when its float64 sum provably decomposes into integer cycle
    + context entries; otherwise the float64 rows (exact path)."""
    from kbbq import _native as N
    from kbbq.gatk import applybqsr as A
    rng = np.random.default_rng(1)
    R, S = 2, 10
    ints = [rng.integers(20, 30, R), rng.integers(-2, 3, R), rng.integers(-3, 4, (R, 43)), rng.integers(-3, 4, (R, 43, 2 * S)),
            np.concatenate([rng.integers(-3, 4, (R, 43, 16)), np.zeros((R, 43, 1), np.int64)], -1)]
    mode, blob, *shape = A._model(*ints, 6)
    assert mode == N.ALIGNED_LUT and shape == [R, 43, 2 * S]
    rs = N.load().kbbq_lut_row_stride(2 * S)
    lut = blob[:R * 43 * rs * 2].view(np.int16).reshape(R, 43, rs)
    assert lut[1, 7, 3] == ints[0][1] + ints[1][1] + ints[2][1, 7] + ints[3][1, 7, 3]
    assert lut[1, 7, 2 * S + 5 * 3 + 2] == ints[4][1, 7, 4 * 3 + 2] and lut[1, 7, 2 * S + 24] == 0
    # the same model in float64 with a non-integer meanq that keeps every sum on the same side of its integer: LUT
    flt = [x.astype(np.float64) for x in ints]
    flt[0] = flt[0] + 0.25
    mode, blob2, *_ = A._model(*flt, 6)
    assert mode == N.ALIGNED_LUT
    assert np.array_equal(blob2.view(np.int16).reshape(R, 43, rs)[..., :2 * S], lut[..., :2 * S])
    # a level a few ulps under an integer, fractions in both the context and the cycle entries: the truncated sums no longer
    # decompose -> float64 rows
    flt[0] = ints[0].astype(np.float64) - 2 ** -40
    flt[3] = flt[3] + np.linspace(0, 0.9, 2 * S)
    flt[4][..., :16] += 0.5
    mode, rows, *_ = A._model(*flt, 6)
    assert mode == N.ALIGNED_F64
    rows = rows.view(np.float64).reshape(R, 43, 18 + 2 * S)
    assert rows[1, 7, 0] == (flt[0][1] + flt[1][1]) + flt[2][1, 7] and np.array_equal(rows[..., 18:], flt[3])


def test_sub_command_arguments(tmp_path, monkeypatch):
    from kbbq import main
    from kbbq.gatk import applybqsr
    seen = {}
    monkeypatch.setattr(applybqsr, 'apply_report', lambda *a, **k: seen.update(args=a, kw=k))
    main.main(['applybqsr', '-b', 'in.bam', '-g', 'r.grp', '-o', 'out.sam', '-u', '-s'])
    assert seen['args'] == ('in.bam', 'r.grp') and seen['kw'] == dict(use_oq=True, set_oq=True, output='out.sam')
    main.main(['applybqsr', '-b', 'in.sam', '--gatkreport', 'r.grp'])
    assert seen['kw'] == dict(use_oq=False, set_oq=False, output=None)
    for bad in (['applybqsr', '-b', 'in.sam'], ['bqsr', '-b', 'in.sam', '-r', 'x.fa', '-g', 'r.grp']):
        with pytest.raises(SystemExit):
            main.main(bad)
    from kbbq.gatk import bqsr
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: seen.update(report=a) or type('R', (), {'write': lambda s, p: seen.update(out=p)})())
    from kbbq import aln, benchmark
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: ('aln', p))
    monkeypatch.setattr(benchmark, 'get_var_sites', lambda p: ('vcf', p))
    main.main(['bqsr', '-b', 'in.sam', '-r', 'x.fa', '-v', 's.vcf', '-g', 'r.grp'])
    assert seen['report'] == (('aln', 'in.sam'), 'x.fa', ('vcf', 's.vcf')) and seen['out'] == 'r.grp'


def test_bam_output_is_refused(tmp_path):
    from kbbq.gatk import applybqsr
    with pytest.raises(ValueError, match='BAM output'):
        applybqsr.apply_report(str(tmp_path / 'missing.sam'), str(tmp_path / 'r.grp'), output=str(tmp_path / 'o.BAM'))
    assert not (tmp_path / 'o.BAM').exists()


def test_new_symbols_are_exported_and_declared():
    from kbbq import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    for name in ('kbbq_apply_aligned_dev', 'kbbq_apply_aligned', 'kbbq_sam_render'):
        assert hasattr(lib, name) and name in N.PROTOTYPES
        assert re.search(r'\bint\s+%s\(' % name, header)
    assert re.search(r'#define KBBQ_ALIGNED_LUT 0', header) and re.search(r'#define KBBQ_ALIGNED_F64 1', header)
