"""
CPU tests of the product's host side: the C ABI library loads and exports every
symbol include/kbbq_hip.h declares, the FASTQ packer, the model numerics
(product code vs oracle and vs reference goldens) and the covariate / read data
classes (restating the reference's tests/test_covariate.py and tests/test_read.py).
No kernel is launched here.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import kbbq
from kbbq import _native, compare_reads, covariate, fastx, read


# ---------------------------------------------------------------- C ABI
def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(kbbq_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) >= 20
    lib = _native.load()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert declared == set(_native.PROTOTYPES), declared ^ set(_native.PROTOTYPES)
    assert lib.kbbq_abi_version() == 1
    assert lib.kbbq_tables_count(2, 300) == 2 * 2 * 43 * 300 + 2 * 2 * 43 * 16
    assert lib.kbbq_lut_count(1, 43, 300) % 2 == 0
    assert lib.kbbq_lut_row_stride(300) == 326


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    with pytest.raises(_native.KbbqHipError):
        _native.Context(0)
    from kbbq import _device
    with pytest.raises(_native.KbbqHipError):
        _device.context()


def test_build_lut_host():
    lib = _native.load()
    R, Qt, S2, D, minscore = 2, 5, 6, 17, 2
    rng = np.random.default_rng(0)
    meanq = rng.integers(0, 40, R); rgdq = rng.integers(-3, 3, R)
    qdq = rng.integers(-3, 3, (R, Qt)); posdq = rng.integers(-5, 5, (R, Qt, S2))
    ddq = rng.integers(-5, 5, (R, Qt, D)); ddq[..., 16] = 0
    rs = lib.kbbq_lut_row_stride(S2)
    assert rs >= S2 + 25 and rs % 2 == 0 and (rs // 2) % 2 == 1
    assert lib.kbbq_lut_count(R, Qt, S2) == R * Qt * rs
    nbytes = lib.kbbq_lut_bytes(R, Qt, S2)
    blob = np.zeros((nbytes + 7) // 8, dtype=np.int64).view(np.uint8)
    a = [np.ascontiguousarray(x, dtype=np.int64) for x in (meanq, rgdq, qdq, posdq, ddq)]
    flags = ctypes.c_int(-1)
    _native.check(lib.kbbq_build_lut(R, Qt, S2, D, minscore, *[_native.ptr(x) for x in a], _native.ptr(blob),
                                     ctypes.byref(flags)))
    rows = blob[:R * Qt * rs * 2].view(np.int16).reshape(R, Qt, rs)
    lut1 = (meanq + rgdq)[:, None, None] + qdq[..., None] + posdq
    assert np.array_equal(rows[..., :S2], lut1)
    for pa in range(5):
        for pb in range(5):
            want = ddq[..., 4 * pa + pb] if pa < 4 and pb < 4 else ddq[..., 16]
            assert np.array_equal(rows[..., S2 + 5 * pa + pb], want)
    assert flags.value == 0
    # table-driven part: rows by raw quality byte
    fb = lib.kbbq_full_lut_bytes(R, Qt, S2)
    off = (R * Qt * rs * 2 + 15) // 16 * 16
    full = blob[off:off + fb].view(np.int8).reshape(R, 33 + Qt, -1)
    W = S2 + 16
    assert np.all(full[:, 0, :2 * W] == -33) and np.all(full[:, 0, 2 * W:] == 0)
    for qb in range(1, 33 + minscore):
        assert np.all(full[:, qb, :2 * W] == qb - 33) and np.all(full[:, qb, 2 * W:] == 0)
    for q in range(minscore, Qt):
        assert np.array_equal(full[:, 33 + q, :S2], lut1[:, q])
        assert np.array_equal(full[:, 33 + q, W:W + S2], lut1[:, q, ::-1])
        assert np.array_equal(full[:, 33 + q, 2 * W:2 * W + 25], rows[:, q, S2:S2 + 25])
    a[3][0, 3, 0] = 300
    _native.check(lib.kbbq_build_lut(R, Qt, S2, D, minscore, *[_native.ptr(x) for x in a], _native.ptr(blob),
                                     ctypes.byref(flags)))
    assert flags.value == 3           # does not fit int8 and can leave 0..255
    with pytest.raises(ValueError):
        _native.check(lib.kbbq_build_lut(R, Qt, S2, 3, minscore, *[_native.ptr(x) for x in a], _native.ptr(blob),
                                         ctypes.byref(flags)))


# ---------------------------------------------------------------- FASTQ packer
def _write(tmp_path, name, recs, end='\n'):
    p = tmp_path / name
    p.write_text(''.join('@%s\n%s\n+\n%s%s' % (r + (end,)) for r in recs))
    return str(p)


def test_pack_pair_matches_oracle(oracle, tmp_path):
    info, _ = load_golden('c5cut_2k_mixed')
    c = info['case']
    seq, cseq, qual, meta = oracle.synth(0, 300, c['n'], c['seed'], c['len_lo'], c['len_hi'], c['nrg'])
    names = oracle.synth_names(0, 300, c['nrg'], with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    want = oracle.pack_records(oracle.read_fastq(fa), oracle.read_fastq(fb), True)
    for packer in (fastx.pack_pair, fastx.pack_pair_py):        # C++ packer and its NumPy twin
        got = packer(fa, fb, True)
        assert got['pending_error'] is None
        assert (got['n'], got['S'], got['R'], got['pitch']) == (want['n'], want['S'], want['R'], want['pitch'])
        for k in ('seq', 'cseq', 'qual', 'meta'):
            assert np.array_equal(got[k], want[k]), k
        assert list(got['rg_to_int']) == want['rg_names']
    got = fastx.pack_pair(fa, fb, True)
    single = fastx.pack_single(got['text'], True)
    assert np.array_equal(single['seq'], want['seq']) and np.array_equal(single['meta'], want['meta'])
    single = fastx.pack_single_py(fastx.FastqText(fa), True)
    assert np.array_equal(single['seq'], want['seq']) and np.array_equal(single['meta'], want['meta'])
    # the C++ writer renders exactly the reference's four lines per record
    text = got['text'].format(0, got['n'], got['qual']).decode('ascii')
    assert text == open(fa).read()
    assert got['text'].format(7, 3, got['qual'][7:10]).decode('ascii') == ''.join(
        '@%s\n%s\n+\n%s\n' % r for r in oracle.read_fastq(fa)[7:10])


def test_fastq_reader_names_comments_and_endings(tmp_path):
    p = tmp_path / 'x.fq'
    p.write_bytes(b'@r1/1 some comment\nACGT\n+r1\nIIII\r\n@r2/2_RG:Z:foo\tcomment\nAC\n+\nII')
    t = fastx.FastqText(str(p))
    assert t.names() == ['r1/1', 'r2/2_RG:Z:foo']
    recs = list(fastx.FastxFile(str(p)))
    assert recs[0].comment == 'some comment' and recs[0].sequence == 'ACGT' and recs[1].quality == 'II'
    assert recs[0].get_quality_array() == [40, 40, 40, 40]
    assert str(recs[1]) == '@r2/2_RG:Z:foo\nAC\n+\nII'
    assert fastx.infer_second('r2/2_RG:Z:foo') and not fastx.infer_second('r2_foo_/2')
    assert fastx.infer_rg('r2/2_RG:Z:foo') == 'foo'
    m, rgmap, err = fastx.make_meta(t.names(), t.lengths(), False)
    assert err is None and list(m) == [4, 2 | (1 << 31)]


@pytest.mark.parametrize('packer', ['native', 'numpy'])
def test_pack_pair_error_ordering(tmp_path, packer):
    pack = fastx.pack_pair if packer == 'native' else fastx.pack_pair_py
    # name mismatch (read 1) comes before the short read (read 2)
    a = _write(tmp_path, 'a.fq', [('x', 'ACGT', 'IIII'), ('y', 'ACGT', 'IIII'), ('z', 'AC', 'II')])
    b = _write(tmp_path, 'b.fq', [('x', 'ACGT', 'IIII'), ('q', 'ACGT', 'IIII'), ('z', 'AC', 'II')])
    p = pack(a, b, False)
    idx, exc, inclusive = p['pending_error']
    assert idx == 1 and isinstance(exc, AssertionError) and not inclusive and p['n'] == 1
    # short read: IndexError, the read itself still goes to the device (its TypeError would win)
    p = pack(a, a, False)
    idx, exc, inclusive = p['pending_error']
    assert idx == 2 and isinstance(exc, IndexError) and inclusive and p['n'] == 3
    # RG inference failure on read 0 wins over everything later
    p = pack(a, b, True)
    assert p['pending_error'][0] == 0 and isinstance(p['pending_error'][1], IndexError)
    # a second field that is not an RG field: AssertionError; length mismatch: ValueError
    r = _write(tmp_path, 'r.fq', [('x/1_RG:Z:a', 'ACGT', 'IIII'), ('y/1_XX:Z:a', 'ACGT', 'IIII')])
    p = pack(r, r, True)
    assert p['pending_error'][0] == 1 and isinstance(p['pending_error'][1], AssertionError) and p['n'] == 1
    m = _write(tmp_path, 'm.fq', [('x', 'ACGT', 'IIII'), ('y', 'ACG', 'III'), ('z', 'AC', 'II')])
    p = pack(a, m, False)
    assert p['pending_error'][0] == 1 and isinstance(p['pending_error'][1], ValueError) and p['n'] == 1
    # zip() truncation
    c = _write(tmp_path, 'c.fq', [('x', 'ACGT', 'IIII')])
    assert pack(a, c, False)['n'] == 1
    # RG ids in first-appearance order, text after the last ':' of the RG field
    g = _write(tmp_path, 'g.fq', [('a/1_RG:Z:b', 'AC', 'II'), ('a/2_RG:Z:b', 'AC', 'II'),
                                   ('c/1_RG:a', 'AC', 'II'), ('d/2_RG:Z:b_x', 'AC', 'II')])
    p = pack(g, g, True)
    assert p['pending_error'] is None and list(p['rg_to_int']) == ['b', 'a']
    assert [int(x) for x in p['meta']] == [2, 2 | (1 << 31), 2 | (1 << 16), 2 | (1 << 31)]


def test_native_fastq_reader_edge_cases(tmp_path):
    p = tmp_path / 'x.fq'
    p.write_bytes(b'@r1/1 some comment\nACGT\n+r1\nIIII\r\n@r2/2_RG:Z:foo\tcomment\nAC\n+\nII')
    f = fastx.NativeFastq(str(p))
    assert f.n == 2 and f.names() == ['r1/1', 'r2/2_RG:Z:foo']
    n, S, R, kind, idx = f.scan(None, False)
    assert (n, S, R, kind) == (2, 4, 1, 0)
    seq, _, qual, meta = f.fill(None, False, 2, 16)
    assert bytes(seq[0]) == b'ACGT' + b'N' * 12 and bytes(qual[1]) == b'II' + bytes(14)
    assert list(meta) == [4, 2 | (1 << 31)]
    assert f.format(0, 2, qual) == b'@r1/1\nACGT\n+\nIIII\n@r2/2_RG:Z:foo\nAC\n+\nII\n'
    empty = tmp_path / 'e.fq'; empty.write_bytes(b'')
    assert fastx.NativeFastq(str(empty)).n == 0
    bad = tmp_path / 'b.fq'; bad.write_bytes(b'@r\nAC\n+\n')
    with pytest.raises(ValueError):
        fastx.NativeFastq(str(bad))


# ---------------------------------------------------------------- model numerics
def test_prior_and_q_p_tables_match_reference():
    info, _ = load_golden('numeric')
    prior = [float(x).hex() if np.isfinite(x) else '-inf' for x in compare_reads.RescaledNormal.prior_dist]
    assert prior == info['prior_dist_hex']
    assert compare_reads.RescaledNormal.prior_dist.dtype == np.longdouble
    assert compare_reads.RescaledNormal.prior(0) == np.log(.9)
    assert np.array_equal(compare_reads.RescaledNormal.prior(np.arange(43)),
                          compare_reads.RescaledNormal.prior_dist)
    q = np.arange(43)
    assert [float(x).hex() for x in compare_reads.q_to_p(q)] == info['q_to_p_hex']
    assert [int(x) for x in compare_reads.p_to_q(compare_reads.q_to_p(q))] == info['p_to_q_of_q_to_p']
    s = info['p_to_q_samples']
    assert [int(x) for x in compare_reads.p_to_q(np.array(s['p']))] == s['q']
    assert np.array_equal(compare_reads.p_to_q(np.array([.2, .3, .4, .1, .01, .001])),
                          np.array([6, 5, 3, 10, 20, 30]))


def test_sequential_constant_sum_is_exact():
    """_solve.sequential_constant_sum == a longdouble accumulator fed one add at a time."""
    from kbbq import _solve
    if np.finfo(np.longdouble).nmant != 63:
        pytest.skip('np.longdouble is not x87 extended here')
    ps = [10.0 ** (-(q / 10.0)) for q in (0, 6, 7, 10, 20, 25, 30, 37, 40, 42)] + [0.5, 0.75, 1.0 / 3, 2.0 ** -20 * 3]
    for p in ps:
        acc = np.longdouble(0); step = np.longdouble(np.float64(p))
        checks = {1, 2, 3, 5, 17, 100, 1023, 1024, 4097, 30000, 65537, 300000}
        for i in range(1, 300001):
            acc = acc + step
            if i in checks:
                assert _solve.sequential_constant_sum(p, i) == acc, (p, i)
    # the mean of n copies of 10^-4 truncates to 39 or 40 depending on the accumulated rounding
    from kbbq import compare_reads
    for n in (2, 1000, 300000, 7_500_000_000):
        s = _solve.sequential_constant_sum(np.float64(1e-4), n)
        assert abs(float(s / n) / 1e-4 - 1) < 1e-9
        assert int(compare_reads.p_to_q(np.array([s / n]))[0]) in (39, 40)


def test_meanq_from_marginals_matches_reference():
    from kbbq import recalibrate
    for name in ('c1_10k_1rg', 'c3cut_2k_8rg', 'c5cut_2k_mixed', 'q42_500_3rg', 'short_64_1rg'):
        _, g = load_golden(name)
        v = recalibrate._vectors_from_tables(g['pos_errs'], g['pos_total'], g['dinuc_errs'],
                                             g['dinuc_total'], 42)
        for k, x in zip(['meanq', 'rg_errs', 'rg_total', 'q_errs', 'q_total'], v):
            assert np.array_equal(x, g[k]), (name, k)


# ---------------------------------------------------------------- covariate helpers
def test_covariate_helpers():
    # reference tests/test_compare_reads.py:130-139, 168-189
    order = ['AA', 'AT', 'AG', 'AC', 'TA', 'TT', 'TG', 'TC', 'GA', 'GT', 'GG', 'GC', 'CA', 'CT', 'CG', 'CC']
    assert order == compare_reads.Dinucleotide.dinucs
    assert np.array_equal(compare_reads.Dinucleotide.vecget(np.array(order)), np.arange(16))
    assert compare_reads.Dinucleotide.vecget(np.array(['AA'])) == 0
    assert np.array_equal(compare_reads.generic_cycle_covariate(17), np.arange(17))
    assert np.array_equal(compare_reads.generic_cycle_covariate(17, True), -(np.arange(17) + 1))
    s = np.array(list('ATGCATGC')); q = np.array([10] * 8)
    want = np.concatenate([[-1], compare_reads.Dinucleotide.vecget(
        np.array(['AT', 'TG', 'GC', 'CA', 'AT', 'TG', 'GC']))])
    assert np.array_equal(compare_reads.generic_dinuc_covariate(s, q), want)
    s[1] = 'N'; want[1] = -1; want[2] = -1
    assert np.array_equal(compare_reads.generic_dinuc_covariate(s, q), want)
    q[6] = 2; want[6] = -1
    assert np.array_equal(compare_reads.generic_dinuc_covariate(s, q), want)
    with pytest.raises(TypeError):
        compare_reads.generic_dinuc_covariate(np.array(list('AcGT')), np.array([10] * 4))
    r = fastx.FastxRecord('foo/2_RG:Z:bar', 'ATG', '((#')
    assert compare_reads.fastq_infer_secondinpair(r) and compare_reads.fastq_infer_rg(r) == 'bar'
    assert np.array_equal(compare_reads.fastq_cycle_covariates(r, True), [-1, -2, -3])
    assert np.array_equal(compare_reads.fastq_dinuc_covariates(r), [-1, 1, -1])


# ---------------------------------------------------------------- covariate classes (reference tests/test_covariate.py)
def test_pad_axis_and_covariate_basics():
    assert np.array_equal(covariate.pad_axis(np.array([1]), 0, 2), [1, 0, 0])
    assert np.array_equal(covariate.pad_axis(np.array([[1]]), 0, 2), [[1], [0], [0]])
    assert np.array_equal(covariate.pad_axis(np.array([[1]]), 1, 2), [[1, 0, 0]])
    t = covariate.Covariate(); assert t.errors.shape == (0,) and t.total.shape == (0,)
    t = covariate.Covariate((1, 2)); assert t.shape() == (1, 2)
    t = covariate.Covariate(); t.pad_axis(0); assert t.shape() == (1,)
    t = covariate.Covariate((3, 4)); t.pad_axis(1, 2); assert t.shape() == (3, 6)
    t = covariate.Covariate(); t.pad_axis_to_fit(0, 99); assert t.shape() == (100,)
    t = covariate.Covariate((1, 2)); t.pad_axis_to_fit(1, -10); assert t.shape() == (1, 10)
    t.pad_axis_to_fit(1, 0); assert t.shape() == (1, 10)
    t = covariate.Covariate((10,)); t.increment((0, 0), (0, 1))
    assert np.array_equal(t.errors, np.zeros(10)) and np.array_equal(t.total, [1] + [0] * 9)
    t = covariate.Covariate((1,)); t[0] = (0, 1); t.increment((0, 0), (0, 1)); assert t[0] == (0, 2)


def test_cyclecovariate_growth_keeps_negative_half():
    t = covariate.CycleCovariate(); assert t.shape() == (0, 0, 0)
    t.pad_axis(axis=0, n=1); assert t.shape() == (1, 0, 0)
    with pytest.raises(ValueError):
        t.pad_axis(2, 1)
    t.pad_axis(1, 1); t.pad_axis(2, 2); assert t.shape() == (1, 1, 2)
    t[(0, 0, 0)] = (1, 1); t[(0, 0, -1)] = (2, 2)
    t.pad_axis(2, 4)
    assert t.shape() == (1, 1, 6) and t[0, 0, 0] == (1, 1) and t[0, 0, -1] == (2, 2)
    c = covariate.CycleCovariate(); c.pad_axis(2, 2); assert c.num_cycles() == 1
    d = covariate.DinucCovariate(); assert d.shape() == (0, 0, 16) and d.num_dinucs() == 16
    cd = covariate.CovariateData()
    assert cd.qcov.shape() == (0, 0) and cd.cyclecov.shape() == (0, 0, 0) and cd.dinuccov.shape() == (0, 0, 16)
    assert (cd.get_num_rgs(), cd.get_num_qs(), cd.get_num_cycles(), cd.get_num_dinucs()) == (0, 0, 0, 16)


@pytest.fixture()
def exreaddata():
    # reference tests/conftest.py:204-218
    yield read.ReadData(seq=np.array(['A', 'T', 'G']), qual=np.array([6, 10, 3]),
                        skips=np.array([False, False, True]), name='read01', rg=0, second=False,
                        errors=np.array([False, True, True]))
    read.ReadData.rg_to_pu = dict(); read.ReadData.rg_to_int = dict(); read.ReadData.numrgs = 0


def test_readdata_getters(exreaddata):
    r = exreaddata
    assert len(r) == 3 and r.get_rg_int() == 0 and r.get_pu() == 0 and r.canonical_name() == 'read01/1'
    assert r.str_qual() == ["'", '+', '$']
    assert np.array_equal(r.not_skipped_errors(), [False, True, False])
    rge, rgv = r.get_rg_errors(); assert list(rge) == [0] and list(rgv) == [0, 0]
    qe, qv = r.get_q_errors(); assert list(qe) == [10] and list(qv) == [6, 10]
    ce, cv = r.get_cycle_errors(); assert list(ce) == [1] and list(cv) == [0, 1]
    assert list(r.get_dinucleotide_array()) == [-1, 1, -1]
    de, dv = r.get_dinuc_errors(); assert list(de) == [1] and list(dv) == [1]
    r.second = True
    assert list(r.get_cycle_array()) == [-1, -2, -3]


def test_readdata_from_fastq():
    rec = fastx.FastxRecord('foo/2_RG:Z:bar', 'ATG', '((#')
    r = read.ReadData.from_fastq(rec)
    assert r.name == 'foo' and r.rg == 'bar' and r.second and list(r.qual) == [7, 7, 2]
    assert not r.skips.any() and not r.errors.any()
    assert read.ReadData.rg_to_int['bar'] == r.get_rg_int()
    read.ReadData.rg_to_pu = dict(); read.ReadData.rg_to_int = dict(); read.ReadData.numrgs = 0


def test_rg_and_q_covariate_consume_read(exreaddata):
    t = covariate.RGCovariate()
    res = t.consume_read(exreaddata)
    assert list(res[0]) == [0] and list(res[1]) == [0, 0] and t[0] == (1, 2) and t.num_rgs() == 1
    q = covariate.QCovariate(); assert q.num_qs() == 0
    (rge, rgv), (qe, qv) = q.consume_read(exreaddata)
    assert list(qe) == [10] and list(qv) == [6, 10] and q[(0, 10)] == (1, 1) and q.num_qs() == 11


def test_dispatcher_errors():
    from kbbq import recalibrate
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate_bam(None)
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate(fastq=None, bam='foo')
    # the reference raises NotImplementedError for any gatkreport (recalibrate.py:167-168, tests/test_recalibrate.py:113-114);
    # here the option is implemented for FASTQ input and every other use of it raises as the reference does
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate(fastq=None, bam=None, gatkreport='foo')
    with pytest.raises(NotImplementedError):
        recalibrate.recalibrate(fastq=None, bam='foo', gatkreport='foo')
    with pytest.raises(ValueError):
        recalibrate.recalibrate(fastq=None, bam=None, gatkreport=None)
    a = fastx.FastxRecord('r', 'ACGTAC', 'IIIIII'); b = fastx.FastxRecord('r', 'ACGTAC', 'IIIIII')
    b.sequence = 'ACGTAG'
    assert list(recalibrate.find_corrected_sites(a, b)) == [False] * 5 + [True]
    with pytest.raises(AssertionError):
        recalibrate.find_corrected_sites(a, fastx.FastxRecord('s', 'ACGTAC', 'IIIIII'))


def test_sharded_packing_concatenates_to_the_whole(oracle, tmp_path):
    """pack_pair / pack_single with shard = (rank, world): every rank scans everything (global read groups,
    longest read, first error) and packs its own contiguous records; pairs stay together."""
    info, _ = load_golden('c5cut_2k_mixed')
    c = info['case']
    n = 301
    seq, cseq, qual, meta = oracle.synth(0, n, c['n'], c['seed'], c['len_lo'], c['len_hi'], c['nrg'])
    names = oracle.synth_names(0, n, c['nrg'], with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    whole = fastx.pack_pair(fa, fb, True)
    for world in (2, 3, 8):
        parts = [fastx.pack_pair(fa, fb, True, shard=(r, world)) for r in range(world)]
        assert [p['first'] for p in parts] == [sum(q['n'] for q in parts[:i]) for i in range(world)]
        assert all(p['first'] % 2 == 0 for p in parts) and sum(p['n'] for p in parts) == whole['n'] == parts[0]['total']
        for k in ('seq', 'cseq', 'qual', 'meta'):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
        assert all((p['S'], p['R'], p['pitch'], p['rg_to_int']) == (whole['S'], whole['R'], whole['pitch'], whole['rg_to_int'])
                   for p in parts)
        singles = [fastx.pack_single(whole['text'], True, shard=(r, world)) for r in range(world)]
        assert np.array_equal(np.concatenate([p['qual'] for p in singles]), whole['qual'])


def _ranks_in_threads(world, fn):
    """fn(rank, gather) on `world` threads with a gather that works like all_gather_object: the results in rank order."""
    import threading
    barrier, box, results, errors = threading.Barrier(world), [None] * world, [None] * world, [None] * world

    def worker(rank):
        def gather(obj):
            box[rank] = obj
            barrier.wait()
            everyone = list(box)
            barrier.wait()
            return everyone
        try:
            results[rank] = fn(rank, gather)
        except Exception as e:               # noqa: BLE001
            errors[rank] = e
    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return results, errors


def test_every_rank_cuts_its_own_byte_range(oracle, tmp_path):
    """The multi-rank opening in which nobody reads a whole file (fastx.local_ranges): byte cuts at record starts (never
    in front of a second-in-pair read), one gather of counts / read groups / longest read / first offender; the ranks'
    packed reads concatenate to the single-process packing, the file-wide facts equal the whole-file scan's."""
    info, _ = load_golden('c5cut_2k_mixed')
    c = info['case']
    n = 1201
    seq, cseq, qual, meta = oracle.synth(0, n, c['n'], c['seed'], c['len_lo'], c['len_hi'], c['nrg'])
    names = oracle.synth_names(0, n, c['nrg'], with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    whole = fastx.pack_pair(fa, fb, True)
    for world in (2, 3, 5, 8):
        parts, errors = _ranks_in_threads(world, lambda r, g: fastx.pack_pair(fa, fb, True, shard=(r, world), gather=g))
        assert not any(errors), errors
        assert [p['first'] for p in parts] == [sum(q['n'] for q in parts[:i]) for i in range(world)]
        assert all(p['first'] % 2 == 0 for p in parts) and sum(p['n'] for p in parts) == whole['n'] == parts[0]['total']
        assert all(p['n'] > 0 for p in parts) and len({p['n'] for p in parts}) > 1          # byte cuts, not equal counts
        for k in ('seq', 'cseq', 'qual', 'meta'):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
        assert all((p['S'], p['R'], p['pitch'], p['rg_to_int']) == (whole['S'], whole['R'], whole['pitch'], whole['rg_to_int'])
                   for p in parts)
        text = b''.join(p['text'].format(p['first'], p['n'], p['qual']) for p in parts)
        assert text == open(fa, 'rb').read()
    # the first offender is a file-wide fact: a read shorter than an earlier one, in another rank's range
    lens = (meta & 0xFFFF).astype(int)
    bad = 900
    lines = open(fa).read().split('\n')
    linesb = open(fb).read().split('\n')
    keep = max(lens[bad] - 9, 1)
    for L in (lines, linesb):
        L[4 * bad + 1] = L[4 * bad + 1][:keep]; L[4 * bad + 3] = L[4 * bad + 3][:keep]
    open(fa, 'w').write('\n'.join(lines)); open(fb, 'w').write('\n'.join(linesb))
    want = fastx.pack_pair(fa, fb, True)
    assert want['pending_error'][0] == bad and isinstance(want['pending_error'][1], IndexError)
    parts, errors = _ranks_in_threads(3, lambda r, g: fastx.pack_pair(fa, fb, True, shard=(r, 3), gather=g))
    assert not any(errors), errors
    for p in parts:
        assert p['pending_error'][0] == bad and isinstance(p['pending_error'][1], IndexError) and p['total'] == want['total']
    assert sum(p['n'] for p in parts) == want['n']
    # ... and when a rank's FIRST read is shorter than the reads of the rank before it
    oracle.write_fastq(fa, names, seq, qual, meta); oracle.write_fastq(fb, names, cseq, qual, meta)
    probe, _ = _ranks_in_threads(2, lambda r, g: fastx.pack_pair(fa, fb, True, shard=(r, 2), gather=g))
    cut = probe[1]['first']
    lines = open(fa).read().split('\n'); linesb = open(fb).read().split('\n')
    keep = max(lens[cut] - 5, 1)
    for L in (lines, linesb):
        L[4 * cut + 1] = L[4 * cut + 1][:keep]; L[4 * cut + 3] = L[4 * cut + 3][:keep]
    open(fa, 'w').write('\n'.join(lines)); open(fb, 'w').write('\n'.join(linesb))
    want = fastx.pack_pair(fa, fb, True)
    parts, errors = _ranks_in_threads(2, lambda r, g: fastx.pack_pair(fa, fb, True, shard=(r, 2), gather=g))
    assert not any(errors), errors
    assert all(p['pending_error'][0] == want['pending_error'][0] == cut for p in parts)
    # files that do not cut alike (the corrected file is shorter): the ranks fall back to rank 0's plan
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names[:800], cseq[:800], qual[:800], meta[:800])
    want = fastx.pack_pair(fa, fb, True)

    def fallback(r, g):
        def exchange(obj):
            return g(obj)[0]
        return fastx.pack_pair(fa, fb, True, shard=(r, 2), gather=g, exchange=exchange)
    parts, errors = _ranks_in_threads(2, fallback)
    assert not any(errors), errors
    assert sum(p['n'] for p in parts) == want['n'] == 800 and parts[0]['total'] == 800
    for k in ('seq', 'cseq', 'qual', 'meta'):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), want[k]), k


def test_gzip_fastq_is_read_like_plain_text(oracle, tmp_path):
    """pysam.FastxFile reads .gz transparently; so does the native reader (zlib, all gzip members)."""
    import gzip
    n = 400
    seq, cseq, qual, meta = oracle.synth(0, n, n, 8, 20, 90, 2)
    names = oracle.synth_names(0, n, 2, with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    want = fastx.pack_pair(fa, fb, True)
    for p in (fa, fb):
        data = open(p, 'rb').read()
        with open(p + '.gz', 'wb') as fh:                     # two concatenated members, as bgzip-style writers produce
            fh.write(gzip.compress(data[:len(data) // 2]) + gzip.compress(data[len(data) // 2:]))
    got = fastx.pack_pair(fa + '.gz', fb + '.gz', True)
    assert got['n'] == want['n'] == n and got['rg_to_int'] == want['rg_to_int']
    for k in ('seq', 'cseq', 'qual', 'meta'):
        assert np.array_equal(got[k], want[k]), k
    assert got['text'].format(0, n, got['qual']) == open(fa, 'rb').read()


def test_cli_without_arguments_and_version(monkeypatch, capfd):
    """reference tests/test_main.py:5-17: no sub-command behaves like the bare program name with anything appended
    (no error, same output); --version prints and exits."""
    import sys
    from kbbq import main
    monkeypatch.setattr(sys, 'argv', ['kbbq'])
    main.main()
    first = capfd.readouterr()
    monkeypatch.setattr(sys, 'argv', ['kbbq-h'])
    main.main()
    assert capfd.readouterr() == first
    monkeypatch.setattr(sys, 'argv', ['kbbq', '--version'])
    with pytest.raises(SystemExit) as e:
        main.main()
    assert e.value.code == 0 and kbbq.__version__ in capfd.readouterr().out
    monkeypatch.setattr(sys, 'argv', ['kbbq', 'recalibrate'])
    with pytest.raises(SystemExit) as e:                     # -b / -f is required
        main.main()
    assert e.value.code == 2


@pytest.mark.parametrize('scan_chunk', [None, 1, 3, 7])
def test_native_packer_agrees_with_numpy_twin_on_random_inputs(tmp_path, monkeypatch, scan_chunk):
    """Differential test: the C++ packer (pack_pair) against the readable NumPy statement of the rules (pack_pair_py)
    on random FASTQ pairs with random defects -- same usable reads, same first offending read and exception class,
    same planes, sidecars and read-group order.  The scan walks chunks of reads in parallel and merges them in read
    order: tiny chunks (KBBQ_SCAN_CHUNK) put the defects on, before and after chunk boundaries."""
    if scan_chunk is not None:
        monkeypatch.setenv('KBBQ_SCAN_CHUNK', str(scan_chunk))
        monkeypatch.setenv('KBBQ_HOST_THREADS', '4')
    rng = np.random.default_rng(77 + (scan_chunk or 0))
    acgt = np.array(list('ACGTN'))
    for case in range(120):
        n = int(rng.integers(0, 40))
        infer = bool(rng.integers(0, 2))
        base_len = int(rng.integers(1, 40))
        lens = np.sort(rng.integers(max(1, base_len - 3), base_len + 4, n)) if rng.random() < 0.7 else rng.integers(1, base_len + 4, n)
        recs_a, recs_b = [], []
        for i in range(n):
            L = int(lens[i])
            seq = ''.join(rng.choice(acgt, L, p=[.24, .24, .24, .24, .04]))
            cseq = ''.join(c if rng.random() > 0.05 else str(rng.choice(acgt[:4])) for c in seq)
            qual = ''.join(chr(33 + int(q)) for q in rng.integers(0, 42, L))
            name = 'r%d/%d' % (i // 2, 1 + (i & 1))
            if infer or rng.random() < 0.3:
                name += '_RG:Z:g%d' % ((i // 2) % 3)
            name_b = name
            defect = rng.random()
            if defect < 0.03:
                name_b = 'x' + name                                   # corrected name does not start with the name
            elif defect < 0.06:
                cseq = cseq[:-1] if L > 1 else cseq + 'A'             # length mismatch between the files
            elif defect < 0.09 and infer:
                name = name_b = name.split('_')[0]                    # no read-group field
            elif defect < 0.12 and infer:
                name = name_b = name.replace('_RG:', '_XG:')          # second field is not an RG tag
            recs_a.append((name, seq, qual)); recs_b.append((name_b, cseq, qual[:len(cseq)].ljust(len(cseq), 'I')))
        if rng.random() < 0.15 and n > 2:
            recs_b = recs_b[:int(rng.integers(1, n))]                 # zip() truncation
        d = tmp_path / ('c%d' % case); d.mkdir()
        fa, fb = _write(d, 'a.fq', recs_a), _write(d, 'b.fq', recs_b)
        got, want = fastx.pack_pair(fa, fb, infer), fastx.pack_pair_py(fa, fb, infer)
        assert (got['n'], got['S'], got['R'], got['pitch']) == (want['n'], want['S'], want['R'], want['pitch']), case
        ge, we = got['pending_error'], want['pending_error']
        assert (ge is None) == (we is None), case
        if ge is not None:
            assert ge[0] == we[0] and type(ge[1]) is type(we[1]) and ge[2] == we[2], (case, ge, we)
        for k in ('seq', 'cseq', 'qual', 'meta'):
            assert np.array_equal(got[k], want[k]), (case, k)
        assert list(got['rg_to_int'])[:len(want['rg_to_int'])] == list(want['rg_to_int']), case


def test_egress_pipeline_orders_items_and_surfaces_the_first_error():
    """kbbq._egress.pipeline: items leave in order; an exception in the source or in any stage is re-raised in the
    caller's thread after every stage thread has drained (no hang on the bounded queues)."""
    from kbbq import _egress
    out = []
    _egress.pipeline(range(50), lambda x: x * 2, lambda x: x + 1, out.append)
    assert out == [2 * i + 1 for i in range(50)]
    _egress.pipeline([], lambda x: x, out.append)
    _egress.pipeline(range(3), out.append)
    assert out[-3:] == [0, 1, 2]

    def boom(x):
        if x == 6:
            raise ValueError('six')
        return x
    for stages in ((boom, lambda x: x, out.append), (lambda x: x, boom, out.append), (lambda x: x, lambda x: x, boom)):
        with pytest.raises(ValueError):
            _egress.pipeline(range(200), *stages)

    def source():
        yield 1
        raise KeyError('source')
    with pytest.raises(KeyError):
        _egress.pipeline(source(), lambda x: x, out.append)
    # round-robin buffers grow on demand and are reused
    made = []
    slots = _egress.Slots(3, lambda nbytes: made.append(nbytes) or np.empty(nbytes, dtype=np.uint8))
    assert slots.get(0, 10) is slots.get(3, 8) and slots.get(1, 10) is not slots.get(0, 10)
    assert slots.get(0, 50).shape[0] == 50 and made == [10, 10, 50]


def test_reader_length_bands_agree_with_the_numpy_statement(tmp_path):
    """NativeFastq.length_bands (C++, over the reader's own length index) against fastx.length_bands (NumPy) on
    ascending, ragged and empty-read inputs, ranges and the too-many-runs case."""
    rng = np.random.default_rng(5)
    for case in range(40):
        n = int(rng.integers(0, 300))
        kind = case % 4
        lens = rng.integers(0 if kind == 3 else 1, 330, n)
        if kind in (0, 3):
            lens = np.sort(lens)
        elif kind == 1:
            lens = np.sort(rng.integers(140, 152, n))
        recs = [('r%d' % i, 'A' * int(L), 'I' * int(L)) for i, L in enumerate(lens)]
        f = fastx.NativeFastq(_write(tmp_path, 'b%d.fq' % case, recs))
        assert f.n == n
        assert f.length_bands() == fastx.length_bands(lens), (case, lens)
        if n > 10:
            lo, m = int(rng.integers(0, n // 2)), int(rng.integers(1, n // 2))
            assert f.length_bands(lo, m) == fastx.length_bands(lens[lo:lo + m]), case
            assert f.length_bands(lo, m, max_bands=2) == fastx.length_bands(lens[lo:lo + m], max_bands=2), case


def test_pair_scan_job_matches_the_step_by_step_reader(tmp_path):
    """fastx.PairScan (both files opened and scanned on the reader's own threads) hands over what NativeFastq +
    scan() give step by step; file A's failure is reported before file B's; a job nobody waits for is cleaned up."""
    recs = [('r%d/%d_RG:Z:g%d' % (i // 2, 1 + (i & 1), (i // 2) % 3), 'ACGTN'[i % 5] * (20 + i // 8), 'I' * (20 + i // 8)) for i in range(64)]
    fa, fb = _write(tmp_path, 'a.fq', recs), _write(tmp_path, 'b.fq', recs[:40])
    for infer in (False, True):
        A, B, info = fastx.PairScan(fa, fb, infer).result()
        a, b = fastx.NativeFastq(fa), fastx.NativeFastq(fb)
        assert (A.n, B.n) == (a.n, b.n) == (64, 40) and info == a.scan(b, infer) and A.rg_names() == a.rg_names()
        assert info[0] == 40 and info[2] == (3 if infer else 1)
        A1, none, info1 = fastx.PairScan(fa, None, infer).result()
        assert none is None and info1 == a.scan(None, infer) and info1[0] == 64
    missing = str(tmp_path / 'missing.fq')
    for pa, pb, where in ((missing, fb, 'missing.fq'), (fa, missing, 'missing.fq'), (missing, str(tmp_path / 'gone.fq'), 'missing.fq')):
        with pytest.raises(ValueError, match=where):
            fastx.PairScan(pa, pb, False).result()
    job = fastx.PairScan(fa, fb, True)
    with pytest.raises(RuntimeError):
        job.result(), job.result()
    del job
    fastx.PairScan(fa, fb, True)             # never waited for: joined and freed by the wrapper's destructor
    import gc
    gc.collect()


def test_planned_sharding_reads_each_byte_range_once(oracle, tmp_path):
    """Multi-GPU ingest: rank 0 opens and scans the pair and hands out a plan (scan result, read-group names, byte
    ranges); the other ranks index only their shard (NativeFastq.open_range).  Emulated here with a mailbox instead of
    a broadcast: the shards concatenate to the whole, a shard's reader answers with file-wide record numbers, a
    compressed pair falls back to every rank reading everything, rank 0's failure reaches the others."""
    import gzip
    n = 5001
    seq, cseq, qual, meta = oracle.synth(0, n, n, 4, 36, 151, 3)
    names = oracle.synth_names(0, n, 3, with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    whole = fastx.pack_pair(fa, fb, True)
    box = {}
    ex = {0: lambda obj: box.setdefault('plan', obj)}
    for world in (2, 3, 7):
        box.clear()
        parts = [fastx.pack_pair(fa, fb, True, shard=(r, world), exchange=ex.get(r, lambda obj: box['plan'])) for r in range(world)]
        for k in ('seq', 'cseq', 'qual', 'meta'):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), (world, k)
        assert all(p['rg_to_int'] == whole['rg_to_int'] and (p['S'], p['R'], p['total']) == (whole['S'], whole['R'], n) for p in parts)
        assert [p['text'].n for p in parts] == [n] + [p['n'] for p in parts[1:]] and all(p['text'].total == n for p in parts)
        last = parts[-1]
        t, i = last['text'], last['first'] + 3
        assert t.first == last['first'] and t.name(i) == whole['text'].name(i)
        assert t.format(i, 2, last['qual'][3:5]) == whole['text'].format(i, 2, last['qual'][3:5])
        assert t.length_bands(last['first'], last['n']) == whole['text'].length_bands(last['first'], last['n'])
        with pytest.raises(ValueError):
            t.name(0)                                            # not this shard's record
    # compressed input: no byte ranges, every rank reads all of it (same planes)
    ga, gb = str(tmp_path / 'a.fq.gz'), str(tmp_path / 'b.fq.gz')
    for src, dst in ((fa, ga), (fb, gb)):
        with open(src, 'rb') as i, gzip.open(dst, 'wb') as o:
            o.write(i.read())
    box.clear()
    parts = [fastx.pack_pair(ga, gb, True, shard=(r, 2), exchange=ex.get(r, lambda obj: box['plan'])) for r in range(2)]
    assert np.array_equal(np.concatenate([p['seq'] for p in parts]), whole['seq']) and parts[1]['text'].n == n
    # a pending error is part of the plan; a file rank 0 cannot open stops every rank with the same exception
    bad = _write(tmp_path, 'bad.fq', [('x', 'ACGT', 'IIII'), ('y', 'ACG', 'III')])
    good = _write(tmp_path, 'good.fq', [('x', 'ACGT', 'IIII'), ('y', 'ACGT', 'IIII')])
    box.clear()
    parts = [fastx.pack_pair(good, bad, False, shard=(r, 2), exchange=ex.get(r, lambda obj: box['plan'])) for r in range(2)]
    assert all(p['pending_error'][0] == 1 and isinstance(p['pending_error'][1], ValueError) for p in parts)
    box.clear()
    for r in range(2):
        with pytest.raises(ValueError, match='missing'):
            fastx.pack_pair(str(tmp_path / 'missing.fq'), good, False, shard=(r, 2), exchange=ex.get(r, lambda obj: box['plan']))


def test_bgzip_fastq_is_inflated_block_parallel(oracle, tmp_path):
    """A bgzip (BGZF) FASTQ -- many independent gzip members with their sizes in the header -- reads like the plain
    file (blocks inflated in parallel by the library); a damaged block is an error, not a crash."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bamwriter
    n = 3000
    seq, cseq, qual, meta = oracle.synth(0, n, n, 3, 40, 100, 2)
    names = oracle.synth_names(0, n, 2, with_rg=True)
    fa = str(tmp_path / 'a.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    raw = open(fa, 'rb').read()
    bz = tmp_path / 'a.fq.gz'
    bz.write_bytes(bamwriter.bgzf(raw, block=20000))
    plain, comp = fastx.NativeFastq(fa), fastx.NativeFastq(str(bz))
    assert comp.n == plain.n == n and not comp.is_plain() and plain.is_plain()
    assert comp.scan(None, True) == plain.scan(None, True)
    a, b = plain.fill(None, True, n, 112), comp.fill(None, True, n, 112)
    assert all(np.array_equal(x, y) for x, y in zip(a, b) if x is not None)
    bad = bytearray(bz.read_bytes()); bad[len(bad) // 2] ^= 0x55
    (tmp_path / 'bad.fq.gz').write_bytes(bytes(bad))
    with pytest.raises(ValueError):
        fastx.NativeFastq(str(tmp_path / 'bad.fq.gz'))


def test_bench_parent_launches_a_child_job_without_touching_the_gpu(monkeypatch, capsys):
    """bench.py --gpus N > 1 without a launcher's environment: the parent composes the torch.distributed.run command
    the driver itself would use, runs it as a CHILD (subprocess, never exec) before importing torch, and relays the
    one JSON line.  (The ranks themselves need GPUs: tests/test_gpu_parity.py::test_bench_launches_its_own_two_rank_job.)"""
    import importlib, subprocess, sys
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    seen = {}

    class Done:
        returncode = 0
        stdout = b'RCCL version banner\n{"metric": "x", "n_gpus": 4}\n'

    def fake_run(cmd, env=None, stdout=None):
        seen['cmd'], seen['env'], seen['torch_loaded'] = cmd, env, 'torch' in sys.modules
        return Done()
    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.delenv('RANK', raising=False)
    torch_mod = sys.modules.pop('torch', None)            # other tests of this process may have imported it
    try:
        rc = bench.main(['--gpus', '4', '--steps', '3', '--warmup', '1', '--reads', '1000', '--no-extra'])
    finally:
        if torch_mod is not None:
            sys.modules['torch'] = torch_mod
    assert rc == 0 and not seen['torch_loaded']
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run'] and '--nnodes=1' in cmd
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4' and cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    tail = cmd[cmd.index(os.path.join(ROOT, 'bench.py')) + 1:]
    assert tail[:6] == ['--gpus', '4', '--steps', '3', '--warmup', '1'] and '--no-extra' in tail
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'
    assert capsys.readouterr().out.strip() == '{"metric": "x", "n_gpus": 4}'
    # a rank (RANK set) with the wrong world size refuses instead of measuring something else
    monkeypatch.setenv('RANK', '0'); monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit):
        bench.main(['--gpus', '4', '--no-extra'])


def test_bench_output_sample_is_the_same_reads_in_every_layout():
    """bench.py --dump-outputs: Resident.outputs() takes the new qualities of one seeded sample of input reads out of one read
    per row and out of mate-pair rows, each as they are and grouped through a permutation -- here on CPU tensors laid out by
    hand (row i of a grouped plane is pair / read perm[i] of the input)."""
    import importlib, sys, types
    import torch
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    n, S, k = 1000, 150, 64
    rng = np.random.default_rng(1)
    want = rng.integers(33, 75, (n, S), dtype=np.uint8)       # new qualities of read i, input order
    want[:, 0], want[:, 1] = np.arange(n) % 256, np.arange(n) // 256

    class ReadBatch:
        perm = None

    class PairBatch:
        perm = None

    def outputs(batch, plane, perm=None):
        r = bench.Resident.__new__(bench.Resident)
        if perm is not None:
            batch.perm, plane = torch.from_numpy(perm), plane[perm]
        r.torch, r.dev, r.batch, r.S, r.n = torch, types.SimpleNamespace(PairBatch=PairBatch), batch, S, n
        r.out, r.tables = torch.from_numpy(plane), types.SimpleNamespace(buf=torch.arange(7, dtype=torch.int64))
        return r.outputs(k)
    rows = np.zeros((n, 160), np.uint8)
    rows[:, :S] = want
    pairs = np.zeros((n // 2, 304), np.uint8)
    pairs[:, :S], pairs[:, S + 1:2 * S + 1] = want[0::2], want[1::2]
    got = [outputs(ReadBatch(), rows), outputs(ReadBatch(), rows, rng.permutation(n)),
           outputs(PairBatch(), pairs), outputs(PairBatch(), pairs, rng.permutation(n // 2))]
    q = got[0]['qualities']
    idx = q[:, 0].astype(np.int64) + 256 * q[:, 1].astype(np.int64)
    assert q.dtype == np.float32 and q.shape == (k, S) and np.array_equal(q, want[idx]) and np.all(np.diff(idx) > 0)
    for g in got:
        assert np.array_equal(g['qualities'], q)
        assert g['tables'].dtype == np.float64 and np.array_equal(g['tables'], np.arange(7))


def test_empty_bgzip_fastq_is_zero_reads(tmp_path):
    """An empty file written by bgzip is ONLY the 28-byte EOF block (isize 0): zero reads, as the reference sees it."""
    eof = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
    for name, data in (('empty.fq.gz', eof), ('empty2.fq.gz', eof + eof)):
        path = tmp_path / name
        path.write_bytes(data)
        f = fastx.NativeFastq(str(path))
        assert f.n == 0
        f.close()


def test_scan_refuses_more_read_groups_than_the_sidecar_holds(tmp_path):
    n = 32800
    recs = ''.join('@r%d/1_RG:Z:g%d\nACGT\n+\nIIII\n' % (i, i) for i in range(n))
    path = tmp_path / 'many.fq'
    path.write_text(recs)
    f = fastx.NativeFastq(str(path))
    with pytest.raises(ValueError, match='32767 read groups'):
        f.scan(f, True)


def test_pmc_traffic_belongs_to_the_current_kernel_sources():
    """profiles/pmc_traffic.json (the HBM bytes per base bench.py's roofline.traffic is computed from) was taken on the
    kernel sources in the tree: after an edit of K1 / K2 re-run scripts/gpu_pmc_r2.sh and commit its pmc_traffic.json --
    until then bench.py prints `traffic: null`, which this test turns into a visible failure instead of a silent one."""
    import json
    import bench
    with open(os.path.join(ROOT, 'profiles', 'pmc_traffic.json')) as fh:
        pmc = json.load(fh)
    assert pmc['kernel_source_sha'] == bench.kernel_source_sha()
    for layout in ('pairs_nib', 'pairs', 'reads'):
        for kernel in ('k1_accumulate', 'k2_apply'):
            assert 1.5 < pmc[layout][kernel]['hbm_bytes_per_base'] < 3.6
    assert bench.pmc_traffic('pairs_nib', 'k2_apply') == pmc['pairs_nib']['k2_apply']['hbm_bytes_per_base']


def test_hipmem_host_tensors_behave_like_the_torch_subset_they_replace():
    """kbbq/_hipmem.py (device memory, page-locked slabs and events for the command line without torch): the host-side half --
    tensors over NumPy memory, slices along the first axis, reinterpreting views, copies -- needs no GPU; the device half is
    exercised by tests/test_gpu_parity.py::test_the_command_line_runs_without_torch."""
    from kbbq import _hipmem as H
    a = np.arange(48, dtype=np.uint8).reshape(6, 8)
    t = H.from_numpy(a)
    assert t.shape == (6, 8) and t.dtype == np.uint8 and t.numel() == 48 and not t.is_cuda and t.device == H.CPU
    assert np.array_equal(t.numpy(), a) and t.numpy().ctypes.data == a.ctypes.data          # no copy
    s = t[2:5]
    assert s.shape == (3, 8) and np.array_equal(s.numpy(), a[2:5]) and s.data_ptr() == a.ctypes.data + 16
    assert t[4:99].shape == (2, 8) and t[5:2].shape == (0, 8)
    with pytest.raises(IndexError):
        t[::2]
    with pytest.raises(IndexError):
        t[1:2, 1:2]
    v = s.view(H.int32)                                                                     # bytes reinterpreted, last axis rescaled
    assert v.shape == (3, 2) and np.array_equal(v.numpy(), a[2:5].view(np.int32))
    assert s.view(24).shape == (24,) and s.view(-1, 4).shape == (6, 4)
    with pytest.raises(ValueError):
        s.view(5, 5)
    z = H.zeros(3, 8, dtype=H.uint8)
    assert not z.numpy().any()
    z.copy_(s)
    assert np.array_equal(z.numpy(), a[2:5])
    z[1:2].copy_(np.full((1, 8), 7, dtype=np.uint8))
    assert z.numpy()[1].tolist() == [7] * 8 and z.numpy()[0].tolist() == a[2].tolist()
    with pytest.raises(ValueError):
        z.copy_(t)
    e = H.empty((4, 2), dtype=H.int64)
    assert e.shape == (4, 2) and e.nbytes == 64 and H.empty_like(e).shape == (4, 2)
    assert e.cpu() is e and e.to('cpu') is e
    with pytest.raises(ValueError):
        H.from_numpy(a[:, ::2])
    assert H._device_of('cuda:3') == H.Device('cuda', 3) and H._device_of(None) == H.CPU


def test_sequential_reader_hands_out_whole_records(oracle, tmp_path):
    """fastx.FastqStream (csrc/fastq_stream.cpp): segments of whole records from a regular file and from a named pipe, a
    follower with the leader's record counts, a spool that receives what was handed out; the incremental scan carries read
    groups and the longest read from segment to segment and finds what the whole-file scan finds."""
    import threading
    n = 3001
    seq, cseq, qual, meta = oracle.synth(0, n, n, 3, 36, 200, 4)
    order = np.argsort(meta & 0xFFFF, kind='stable')
    seq, cseq, qual, meta = seq[order], cseq[order], qual[order], meta[order]
    names = oracle.synth_names(0, n, 4, with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, [x + '_c' for x in names], cseq, qual, meta)
    whole = open(fa, 'rb').read()
    A, B = fastx.NativeFastq(fa), fastx.NativeFastq(fb)
    want = A.scan(B, True)
    for max_bytes in (1 << 16, 200000, 1 << 30):
        s, t = fastx.FastqStream(fa), fastx.FastqStream(fb)
        assert s.regular
        got, rgs, longest, nseg = b'', [], 0, 0
        while True:
            a, end = s.next(max_bytes)
            if a is None:
                break
            b, _ = t.next(max_bytes, a.n)
            assert b.n == a.n and b.first == a.first
            info = a.scan_next(b, True, rgs, longest)
            assert info[0] == a.n and info[3] == 0
            rgs, longest = a.rg_names(), max(longest, info[1])
            _, _, ql, _ = a.fill(None, True, a.n, 208, first=a.first)
            got += a.format(a.first, a.n, ql)
            nseg += 1
        assert got == whole and rgs == A.rg_names() and longest == want[1] and len(rgs) == want[2]
        assert nseg == (1 if max_bytes > len(whole) else -(-len(whole) // max_bytes)) or nseg >= len(whole) // (max_bytes + 70000)
    # the first offender of a later segment: a read shorter than the longest read of the segments before it
    lines = whole.split(b'\n')
    k = 2500
    lines[4 * k + 1] = lines[4 * k + 1][:20]; lines[4 * k + 3] = lines[4 * k + 3][:20]
    bad = str(tmp_path / 'bad.fq')
    open(bad, 'wb').write(b'\n'.join(lines))
    linesb = open(fb, 'rb').read().split(b'\n')
    linesb[4 * k + 1] = linesb[4 * k + 1][:20]; linesb[4 * k + 3] = linesb[4 * k + 3][:20]
    badb = str(tmp_path / 'badb.fq')
    open(badb, 'wb').write(b'\n'.join(linesb))
    s, t = fastx.FastqStream(bad), fastx.FastqStream(badb)
    rgs, longest, found = [], 0, None
    while found is None:
        a, _ = s.next(100000)
        b, _ = t.next(100000, a.n)
        info = a.scan_next(b, True, rgs, longest)
        rgs, longest = a.rg_names(), max(longest, info[1])
        if info[3]:
            found = (info[3], a.first + info[4], info[0])
    assert found[0] == 5 and found[1] == k and fastx.NativeFastq(bad).scan(fastx.NativeFastq(badb), True)[3:] == [5, k]
    # a named pipe: not regular, read once, teed into a spool
    fifo = str(tmp_path / 'fifo')
    os.mkfifo(fifo)
    th = threading.Thread(target=lambda: open(fifo, 'wb').write(whole))
    th.start()
    s = fastx.FastqStream(fifo)
    assert not s.regular and fastx.is_sequential_input(fifo) and not fastx.is_sequential_input(fa) and fastx.is_sequential_input('-')
    spool = os.open(str(tmp_path / 'spool'), os.O_RDWR | os.O_CREAT)
    s.tee(spool)
    total = 0
    while True:
        a, _ = s.next(150000)
        if a is None:
            break
        total += a.n
    th.join(); os.close(spool)
    assert total == n and open(str(tmp_path / 'spool'), 'rb').read() == whole
    # ends: no last newline, CRLF, an input that stops inside a record, nothing at all, a shorter follower, gzip bytes
    for text, count in ((whole[:-1], n), (whole.replace(b'\n', b'\r\n'), n), (b'', 0)):
        p = str(tmp_path / 'x.fq'); open(p, 'wb').write(text)
        s, total = fastx.FastqStream(p), 0
        while True:
            a, _ = s.next(90000)
            if a is None:
                break
            assert a.name(a.first) == names[a.first]
            total += a.n
        assert total == count
    p = str(tmp_path / 'y.fq'); open(p, 'wb').write(b'\n'.join(whole.split(b'\n')[:4 * 100 + 2]) + b'\n')
    s = fastx.FastqStream(p)
    with pytest.raises(ValueError):
        while s.next(1 << 30)[0] is not None:
            pass
    p = str(tmp_path / 'z.fq'); open(p, 'wb').write(b'\n'.join(open(fb, 'rb').read().split(b'\n')[:4 * 700]) + b'\n')
    s, t, na, nb = fastx.FastqStream(fa), fastx.FastqStream(p), 0, 0
    while True:
        a, _ = s.next(120000)
        if a is None:
            break
        b, _ = t.next(120000, a.n)
        na, nb = na + a.n, nb + (b.n if b is not None else 0)
    assert (na, nb) == (n, 700)
    # gzip / bgzip bytes are inflated as they are read: one member, many members (bgzip), through a pipe; damage is reported
    import gzip
    p = str(tmp_path / 'g.fq.gz'); gzip.open(p, 'wb').write(whole)
    cut = len(whole) // 3
    cut = whole.index(b'\n@', cut) + 1                          # (members need not end at record ends; this one happens to end at a line end)
    p2 = str(tmp_path / 'm.fq.gz')
    open(p2, 'wb').write(gzip.compress(whole[:cut]) + gzip.compress(whole[cut:cut + 100]) + gzip.compress(whole[cut + 100:]) + b'\0' * 40)
    import bamwriter                                            # BGZF blocks (bgzip): inflated many at a time
    p3 = str(tmp_path / 'b.fq.gz'); open(p3, 'wb').write(bamwriter.bgzf(whole, block=0x3000))
    for path in (p, p2, p3):
        s, got = fastx.FastqStream(path), b''
        assert s.regular                                        # compressed, but small (or inflated on all threads): pass 2 reads the file again, no spool
        while True:
            a, _ = s.next(200000)
            if a is None:
                break
            _, _, ql, _ = a.fill(None, False, a.n, 208, first=a.first)
            got += a.format(a.first, a.n, ql)
        assert got == whole
    fifo2 = str(tmp_path / 'fifo_gz')
    os.mkfifo(fifo2)
    th = threading.Thread(target=lambda: open(fifo2, 'wb').write(open(p2, 'rb').read()))
    th.start()
    s, total = fastx.FastqStream(fifo2), 0
    while True:
        a, _ = s.next(150000)
        if a is None:
            break
        total += a.n
    th.join()
    assert total == n
    raw = open(p, 'rb').read()
    bz = open(p3, 'rb').read()
    for name, data in (('cut', raw[:len(raw) // 2]), ('flip', raw[:len(raw) // 2] + bytes([raw[len(raw) // 2] ^ 0x5A]) + raw[len(raw) // 2 + 1:]), ('magic', b'\x1f\x8b'),
                       ('bgzf_cut', bz[:len(bz) // 2]), ('bgzf_flip', bz[:len(bz) // 2] + bytes([bz[len(bz) // 2] ^ 0x5A]) + bz[len(bz) // 2 + 1:])):
        bad = str(tmp_path / (name + '.gz')); open(bad, 'wb').write(data)
        with pytest.raises(ValueError):
            s = fastx.FastqStream(bad)
            while s.next(1 << 20)[0] is not None:
                pass
    # which inputs are read sequentially: pipes, stdin, and compressed files from KBBQ_GZ_STREAM_BYTES on
    assert not fastx.is_sequential_input(p)
    os.environ['KBBQ_GZ_STREAM_BYTES'] = '1000'
    try:
        assert fastx.is_sequential_input(p) and not fastx.is_sequential_input(fa)
    finally:
        del os.environ['KBBQ_GZ_STREAM_BYTES']


def _wrapped(path_in, path_out, width, plus_name=False):
    """The same records with sequence and quality lines wrapped at `width` characters (and the name repeated on the '+' line)."""
    recs = open(path_in).read().split('\n')
    out = []
    for i in range(0, len(recs) - 3, 4):
        h, s_, _, q = recs[i:i + 4]
        out.append(h)
        out += [s_[k:k + width] for k in range(0, max(len(s_), 1), width)]
        out.append('+' + (h[1:] if plus_name else ''))
        out += [q[k:k + width] for k in range(0, max(len(q), 1), width)]
    open(path_out, 'w').write('\n'.join(out) + '\n')


def test_wrapped_fastq_reads_like_four_line_fastq(oracle, tmp_path):
    """Sequence and quality over several lines each (what kseq / pysam.FastxFile accepts, recalibrate.py:56): the mapped reader
    unwraps such a file and packs the same planes, sidecars and names as from the four-line file -- quality lines that begin
    with '@' or '+' included; what kseq refuses stays refused with the four-line reader's message."""
    n = 2000
    seq, cseq, qual, meta = oracle.synth(0, n, n, 6, 36, 150, 3)
    order = np.argsort(meta & 0xFFFF, kind='stable')
    seq, cseq, qual, meta = seq[order], cseq[order], qual[order], meta[order]
    qual[5, 0] = ord('@'); qual[6, 0] = ord('+'); qual[7, 60] = ord('@')          # '@' = Q31, '+' = Q10: legal qualities at line starts
    names = oracle.synth_names(0, n, 3, with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    want = fastx.pack_pair(fa, fb, True)
    for width, plus_name in ((60, False), (7, True), (1000, True)):
        wa, wb = str(tmp_path / ('wa%d.fq' % width)), str(tmp_path / ('wb%d.fq' % width))
        _wrapped(fa, wa, width, plus_name); _wrapped(fb, wb, width, plus_name)
        got = fastx.pack_pair(wa, wb, True)
        assert (got['n'], got['S'], got['R'], got['rg_to_int']) == (want['n'], want['S'], want['R'], want['rg_to_int'])
        for k in ('seq', 'cseq', 'qual', 'meta'):
            assert np.array_equal(got[k], want[k]), (width, k)
        assert got['text'].format(0, n, got['qual']) == open(fa, 'rb').read()             # records leave as four lines
    for text in ('@r1\nACGT\nAC\n+\nIIII\n', '@r1\nACGT\nACGT\n', '@r1\nAC\nGT\n+\nIIIII\nI\n', 'x\n@r1\nAC\nGT\n+\nII\nII\n'):
        p = str(tmp_path / 'bad.fq'); open(p, 'w').write(text)
        with pytest.raises(ValueError):
            fastx.NativeFastq(p)


def test_streaming_helpers_without_a_device(oracle, tmp_path):
    """The host-only pieces of the streamed file path (kbbq/recalibrate.py, kbbq/_stream.py, kbbq/_device.py): byte-size parsing,
    slab sizing, the prefetching iterator (order, an exception of the producer, a consumer that stops early) and the pairing of
    a leading and a following sequential reader segment by segment."""
    import threading
    import time
    from kbbq import _device as D, recalibrate, _stream
    assert [D.parse_bytes(x) for x in ('1024', '64k', '256M', '1.5G', '2GB', '1e6')] == [1024, 65536, 256 << 20, 3 << 29, 2 << 30, 1000000]
    assert _stream.slab_reads(256 << 20, 484) % 2 == 0 and 400000 < _stream.slab_reads(256 << 20, 484) < 450000
    assert _stream.slab_reads(1, 10 ** 9) == 2 and _stream.resident_bytes(10, 150) == 10 * 644
    assert fastx._too_large(8_000_000, 150, 256 << 20) and not fastx._too_large(1000, 150, 256 << 20)
    # order, and one item read ahead
    made = []

    def numbers(n, fail_at=None):
        for i in range(n):
            if i == fail_at:
                raise RuntimeError('producer failed at %d' % i)
            made.append(i)
            yield i
    assert list(recalibrate._prefetched(numbers(50))) == list(range(50))
    with pytest.raises(RuntimeError, match='failed at 7'):
        list(recalibrate._prefetched(numbers(20, fail_at=7)))
    del made[:]
    it = recalibrate._prefetched(numbers(1000))
    assert [next(it) for _ in range(3)] == [0, 1, 2]
    it.close()                                               # joins the producer: nothing is made afterwards
    n_made = len(made)
    time.sleep(0.05)
    assert len(made) == n_made <= 6 and threading.active_count() < 20
    # leader / follower pairing over real sequential readers, the follower ending early and exactly at a segment's end
    n = 3000
    seq, cseq, qual, meta = oracle.synth(0, n, n, 2, 100, 100, 2)
    names = oracle.synth_names(0, n, 2, with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    for keep in (n, 1777, 0):
        oracle.write_fastq(fb, names[:keep], cseq[:keep], qual[:keep], meta[:keep])
        sa, sb = fastx.FastqStream(fa), fastx.FastqStream(fb)
        na = nb = 0
        for a, b in recalibrate._pair_segments(sa, sb, 1 << 16):
            assert b is None or (b.first == a.first and b.n <= a.n)
            na, nb = na + a.n, nb + (b.n if b is not None else 0)
        assert (na, nb) == (n, keep)
    sa = fastx.FastqStream(fa)
    assert sum(a.n for a, b in recalibrate._pair_segments(sa, None, 1 << 16) if b is None) == n


def test_fast_exit_reports_a_failed_flush():
    """main._leave (the single-process command's os._exit): output that cannot be flushed must not end in status 0."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); from kbbq import main; sys.stdout.write('x' * 100); main._leave(); sys.exit(7)"
            % os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kbbq-py_amd'))
    with open('/dev/full', 'wb') as full:
        r = subprocess.run([sys.executable, '-c', code], stdout=full, stderr=subprocess.PIPE)
    assert r.returncode == 120, (r.returncode, r.stderr)
    r = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == b'x' * 100


def test_libdeflate_and_zlib_inflate_alike(oracle, tmp_path):
    """csrc/fast_inflate.h: BGZF blocks and whole gzip files go through libdeflate when the machine has it, through zlib otherwise
    (KBBQ_LIBDEFLATE=0) -- same text, same records, the same error for the same damage (zlib decides what a damaged input is in
    both).  gzip files: one member, two members, highly compressible (the output buffer has to grow), BGZF with an empty block."""
    import gzip
    import hashlib
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bamwriter
    n = 2000
    seq, cseq, qual, meta = oracle.synth(0, n, n, 5, 60, 150, 1)
    fa = str(tmp_path / 'a.fq')
    oracle.write_fastq(fa, oracle.synth_names(0, n, 1, with_rg=False), seq, qual, meta)
    raw = open(fa, 'rb').read()
    cut = raw.index(b'\n@', len(raw) // 2) + 1
    files = {'one.fq.gz': gzip.compress(raw), 'two.fq.gz': gzip.compress(raw[:cut]) + gzip.compress(raw[cut:]),
             'bgzf.fq.gz': bamwriter.bgzf(raw, block=9000),
             'flat.fq.gz': gzip.compress(b''.join(b'@r%d\n%s\n+\n%s\n' % (i, b'A' * 5000, b'I' * 5000) for i in range(300)))}
    damaged = bytearray(files['bgzf.fq.gz']); damaged[len(damaged) // 3] ^= 0x41
    files['bad_block.fq.gz'] = bytes(damaged)
    files['cut.fq.gz'] = files['one.fq.gz'][:len(files['one.fq.gz']) // 2]
    files['tail.fq.gz'] = files['one.fq.gz'] + b'garbage'
    for name, blob in files.items():
        (tmp_path / name).write_bytes(blob)
    code = ('import sys, hashlib; sys.path.insert(0, %r)\n'
            'from kbbq import fastx\n'
            'for p in sys.argv[1:]:\n'
            '    try:\n'
            '        r = fastx.NativeFastq(p)\n'
            '        h = hashlib.sha256()\n'
            '        for i in (0, r.n // 2, r.n - 1):\n'
            '            h.update(r.name(i).encode())\n'
            '        planes = r.fill(None, False, r.n, fastx.pitch_for(int(r.lengths().max())))\n'
            '        for x in planes:\n'
            '            if x is not None: h.update(x.tobytes())\n'
            '        print(p.rsplit("/", 1)[1], r.n, h.hexdigest()[:16])\n'
            '    except Exception as e:\n'
            '        print(p.rsplit("/", 1)[1], type(e).__name__, str(e).rsplit("/", 1)[-1])\n' % os.path.join(ROOT, 'kbbq-py_amd'))
    paths = [str(tmp_path / k) for k in sorted(files)]
    outs = []
    for env in ({}, {'KBBQ_LIBDEFLATE': '0'}):
        r = subprocess.run([sys.executable, '-c', code] + paths, capture_output=True, env=dict(os.environ, **env), timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(r.stdout.decode())
    assert outs[0] == outs[1], outs
    lines = dict(l.split(' ', 1) for l in outs[0].splitlines())
    assert lines['one.fq.gz'] == lines['two.fq.gz'] == lines['bgzf.fq.gz'] and lines['one.fq.gz'].startswith('%d ' % n)
    assert lines['flat.fq.gz'].startswith('300 ')
    assert all(lines[k].startswith('ValueError') for k in ('bad_block.fq.gz', 'cut.fq.gz', 'tail.fq.gz')), lines


def test_gzip_members_inflate_on_many_threads(oracle, tmp_path):
    """csrc/parallel_gunzip.cpp: one gzip member cut into chunks, block starts searched, chunks decoded against an unknown window and
    resolved in order -- through the mapped reader (the whole file) and the sequential reader (window by window), with chunks small
    enough that a test file has dozens; against the plain file and against zlib (KBBQ_PGZ_MIN_BYTES too large for the file).  Every
    compression level, two members, a stored member, a damaged and a truncated file (zlib words the error), and the way back to zlib in
    mid-stream (KBBQ_PGZ_TEST_FAIL_AFTER: the text handed out before is skipped)."""
    import gzip
    import subprocess
    import sys
    n = 6000
    seq, cseq, qual, meta = oracle.synth(0, n, n, 7, 80, 150, 1)
    fa = str(tmp_path / 'a.fq')
    oracle.write_fastq(fa, oracle.synth_names(0, n, 1, with_rg=False), seq, qual, meta)
    raw = open(fa, 'rb').read()
    cut = raw.index(b'\n@', len(raw) // 2) + 1
    files = {'l1.fq.gz': gzip.compress(raw, 1), 'l6.fq.gz': gzip.compress(raw, 6), 'l9.fq.gz': gzip.compress(raw, 9),
             'l0.fq.gz': gzip.compress(raw, 0), 'two.fq.gz': gzip.compress(raw[:cut], 6) + gzip.compress(raw[cut:], 4)}
    import zlib
    z = zlib.compressobj(6, zlib.DEFLATED, 31)               # what pigz writes: empty stored blocks (sync flushes) between stretches
    files['l6sync.fq.gz'] = b''.join(z.compress(raw[i:i + 50000]) + z.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(raw), 50000)) + z.flush()
    damaged = bytearray(files['l6.fq.gz']); damaged[len(damaged) // 2] ^= 0x08
    files['bad.fq.gz'] = bytes(damaged)
    files['cut.fq.gz'] = files['l6.fq.gz'][:len(files['l6.fq.gz']) * 2 // 3]
    for name, blob in files.items():
        (tmp_path / name).write_bytes(blob)
    code = ('import sys, hashlib; sys.path.insert(0, %r)\n'
            'from kbbq import fastx\n'
            'def digest(r, h):\n'
            '    planes = r.fill(None, False, r.n, 160, first=r.first)\n'
            '    for x in planes:\n'
            '        if x is not None: h.update(x.tobytes())\n'
            '    h.update(("%%d %%s %%s" %% (r.n, r.name(r.first), r.name(r.first + r.n - 1))).encode())\n'
            'for p in sys.argv[1:]:\n'
            '    for mode in ("mapped", "stream"):\n'
            '        h = hashlib.sha256(); total = 0\n'
            '        try:\n'
            '            if mode == "mapped":\n'
            '                r = fastx.NativeFastq(p); digest(r, h); total = r.n\n'
            '            else:\n'
            '                s = fastx.FastqStream(p)\n'
            '                while True:\n'
            '                    seg, end = s.next(300000)\n'
            '                    if seg is None: break\n'
            '                    digest(seg, h); total += seg.n\n'
            '            print(p.rsplit("/", 1)[1], mode, total, h.hexdigest()[:16] if mode == "mapped" else "")\n'
            '        except Exception as e:\n'
            '            print(p.rsplit("/", 1)[1], mode, type(e).__name__, str(e).rsplit("/", 1)[-1])\n' % os.path.join(ROOT, 'kbbq-py_amd'))
    paths = [fa] + [str(tmp_path / k) for k in sorted(files)]
    runs = {}
    for label, env in (('zlib', {'KBBQ_PGZ_MIN_BYTES': '1000000000', 'KBBQ_LIBDEFLATE': '0'}),
                       ('threads', {'KBBQ_PGZ_MIN_BYTES': '0', 'KBBQ_PGZ_CHUNK': '20000', 'KBBQ_HOST_THREADS': '4'}),
                       ('tiny chunks', {'KBBQ_PGZ_MIN_BYTES': '0', 'KBBQ_PGZ_CHUNK': '3000', 'KBBQ_HOST_THREADS': '3'}),
                       ('back to zlib', {'KBBQ_PGZ_MIN_BYTES': '0', 'KBBQ_PGZ_CHUNK': '20000', 'KBBQ_HOST_THREADS': '2', 'KBBQ_PGZ_TEST_FAIL_AFTER': '2'})):
        r = subprocess.run([sys.executable, '-c', code] + paths, capture_output=True, env=dict(os.environ, **env), timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        runs[label] = r.stdout.decode()
    assert runs['threads'] == runs['zlib'] == runs['tiny chunks'] == runs['back to zlib'], runs
    lines = runs['zlib'].splitlines()
    good = [l.split(' ', 2)[2] for l in lines if l.startswith(('a.fq ', 'l0', 'l1', 'l6', 'l9', 'two')) and ' mapped ' in l]   # ('l6' takes l6sync too)
    assert len(set(good)) == 1 and good[0].startswith('%d ' % n), lines
    assert all('ValueError' in l for l in lines if l.startswith(('bad', 'cut'))), lines


def test_the_writer_reserves_blocks_without_moving_the_files_end(tmp_path):
    """_egress._Reserve: fallocate(KEEP_SIZE) ahead of every slab's write -- the file holds exactly what was written, sinks that are not
    regular files are left alone, KBBQ_FALLOCATE=0 turns it off, and a refusal ends it quietly."""
    import io
    from kbbq import _egress
    p = tmp_path / 'out.bin'
    with open(p, 'wb') as fh:
        fh.write(b'head')
        r = _egress._Reserve(fh)
        assert r.fd is not None and r.at == 4
        for blob in (b'x' * 100000, b'y' * 5):
            r.ahead(len(blob)); fh.write(blob)
        assert r.at == 4 + 100005
    assert p.read_bytes() == b'head' + b'x' * 100000 + b'y' * 5
    assert _egress._Reserve(io.BytesIO()).fd is None
    rd, wr = os.pipe()
    with os.fdopen(wr, 'wb') as w:
        assert _egress._Reserve(w).fd is None
    os.close(rd)
    os.environ['KBBQ_FALLOCATE'] = '0'
    try:
        with open(p, 'wb') as fh:
            assert _egress._Reserve(fh).fd is None
    finally:
        del os.environ['KBBQ_FALLOCATE']
    with open(p, 'wb') as fh:
        r = _egress._Reserve(fh)
        r.call = lambda *a: -1                                    # a filesystem that refuses
        r.ahead(10)
        assert r.fd is None and r.at == 10
        r.ahead(10)                                               # stays off
        assert r.at == 20


def test_segment_buffers_are_kept_between_segments_and_dropped_with_the_last_stream(oracle, tmp_path):
    """csrc/fastq_stream.cpp kbbq_text_pool_*: a closed segment's buffer serves the next segment (same memory), and nothing is kept once
    no stream is open."""
    n = 3000
    seq, cseq, qual, meta = oracle.synth(0, n, n, 9, 100, 100, 1)
    fa = str(tmp_path / 'a.fq')
    oracle.write_fastq(fa, oracle.synth_names(0, n, 1, with_rg=False), seq, qual, meta)
    s = fastx.FastqStream(fa)
    seg, _ = s.next(100000)
    where = seg.record_offset(seg.first)                              # offsets are relative: ask the library where the text lives
    lib = _native.load()
    p1 = ctypes.c_void_p(); ln = ctypes.c_int(0)
    lib.kbbq_fastq_name(seg._h, 0, ctypes.byref(p1), ctypes.byref(ln))
    first_addr = p1.value
    total = seg.n
    seg.close()
    seg2, _ = s.next(100000)
    lib.kbbq_fastq_name(seg2._h, 0, ctypes.byref(p1), ctypes.byref(ln))
    assert p1.value == first_addr                                     # the same buffer, filled again
    total += seg2.n
    while True:
        seg2.close()
        seg2, _ = s.next(100000)
        if seg2 is None:
            break
        total += seg2.n
    assert total == n
    s.close()
