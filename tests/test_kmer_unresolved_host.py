"""`kbbq bqsr --kmers --skip-unresolved`, no GPU: the CPU model of the three outcomes of the k-mer rule
(tests/kmer_unresolved_model.py) on hand-made reads whose classes are known by construction, the model against
kmer_model.correct and kmer_bqsr_model.vectors where they must agree, the command line's new option, and the new C ABI symbol."""
import os
import re

import numpy as np
import pytest

import kmer_model as M
import kmer_unresolved_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 15
T = 3                                                    # six copies of the genome: every k-mer of it is counted 6 times


def _genome(n=200, seed=3):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, n)])


def _sub(read, *at):
    x = bytearray(read)
    for i in at:
        x[i] = b'ACGT'[(b'ACGT'.index(x[i]) + 1) % 4]
    return bytes(x)


def _last_row(extra):
    """The classes of `extra` beside six copies of the genome, and its two counts."""
    seq, meta = M.plane([_genome()] * 6 + [extra])
    cls, ones, twos, t = U.classify(seq, meta, K, T)
    assert t == T and not cls[:6].any() and not ones[:6].any() and not twos[:6].any()        # the genome itself is trusted
    assert set(np.unique(cls).tolist()) <= {0, 1, 2}
    assert not cls[6, len(extra):].any()                                                      # padding
    assert ones[6] == (cls[6] == 1).sum() and twos[6] == (cls[6] == 2).sum()
    return cls[6, :len(extra)].tolist()


def test_two_substitutions_five_apart_are_both_unresolved():
    """A read of 24 bases has the windows 0..9 at k = 15, and every one of them holds base 9 AND base 14: with both substituted
    no single substitution makes any window solid.  The other bases are untrusted too, and no substitution helps them either."""
    g = _genome()
    got = _last_row(_sub(g[40:64], 9, 14))
    assert got[9] == 2 and got[14] == 2
    assert got == [2] * 24


def test_one_substitution_is_an_error():
    """The same read with base 9 alone substituted: writing the genome's letter back makes all ten windows solid.  Every other
    base is covered by those ten windows only, none solid, and no substitution of its own repairs them."""
    g = _genome()
    got = _last_row(_sub(g[40:64], 9))
    assert got[9] == 1
    assert got == [2] * 9 + [1] + [2] * 14


def test_in_a_long_read_each_of_two_substitutions_has_windows_of_its_own():
    """60 bases, substitutions at 30 and 35: windows 16..20 hold base 30 alone and 31..35 base 35 alone, so each has a strict
    winner; the four bases between them are covered only by windows that hold one of the two -- unresolved."""
    g = _genome()
    got = _last_row(_sub(g[100:160], 30, 35))
    assert got == [0] * 30 + [1] + [2] * 4 + [1] + [0] * 24


def test_unrelated_bases_are_unresolved_wherever_a_window_covers_them():
    rng = np.random.default_rng(99)
    other = bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, 60)])
    assert _last_row(other) == [2] * 60
    # ... with an N at 20: bases 0..19 and 21..59 each still have a window (20 >= k, 39 >= k), the N itself is a break
    assert _last_row(other[:20] + b'N' + other[21:]) == [2] * 20 + [0] + [2] * 39
    # ... and at 10: no window fits in front of it, so bases 0..9 are covered by none and trusted
    assert _last_row(other[:10] + b'N' + other[11:]) == [0] * 11 + [2] * 49


def test_shorter_than_k_has_no_window():
    g = _genome()
    for L in (1, K - 1):
        assert _last_row(_sub(g[10:10 + L], L // 2)) == [0] * L


def test_exactly_k_has_one_window():
    g = _genome()
    assert _last_row(_sub(g[10:10 + K], 7)) == [2] * 7 + [1] + [2] * 7
    assert _last_row(_sub(g[10:10 + K], 0, K - 1)) == [2] * K
    assert _last_row(g[10:10 + K]) == [0] * K


def test_a_substitution_next_to_an_n():
    """N at 15 in a read of 40: window 0 is the only one in front of the N, windows 16..25 the ones behind it (all solid)."""
    g = _genome()
    r = g[60:100]
    one = _sub(r, 14)
    assert _last_row(one[:15] + b'N' + one[16:]) == [2] * 14 + [1] + [0] + [0] * 24
    two = _sub(r, 9, 14)
    assert _last_row(two[:15] + b'N' + two[16:]) == [2] * 15 + [0] + [0] * 24


def test_class_1_is_where_kmer_model_correct_changes_a_base():
    seq, meta = M.synth(5, genome_len=1500, depth=20, err=0.03, len_lo=20, len_hi=120)[:2]
    for k, t in ((15, None), (21, 3)):
        out, changed, tt = M.correct(seq, meta, k, t)
        cls, ones, twos, t2 = U.classify(seq, meta, k, t)
        assert t2 == tt
        assert np.array_equal(cls == 1, out != seq) and np.array_equal(ones, changed)
        assert int(ones.sum()) >= 50 and int(twos.sum()) >= 50
        assert np.array_equal(twos, (cls == 2).sum(axis=1))
        codes = M._codes(seq, meta)
        assert (codes[cls != 0] < 4).all()               # only A/C/G/T inside the read is ever 1 or 2
        # a given solid set is the same judgement
        keys, counts = M.count(seq, meta, k)
        again = U.classify(seq, meta, k, tt, solid_keys=keys[counts >= tt])
        assert np.array_equal(again[0], cls)


def test_vectors_are_the_bqsr_model_with_the_unresolved_bases_taken_out(tmp_path):
    """Against kmer_bqsr_model.vectors: errors are its errors given the class-1 plane; a tally's error vectors given the class-2
    plane instead count the class-2 bases the tally sees per cell, and those are exactly what leaves the totals."""
    import kmer_bqsr_model as B
    import oracle_bqsr as OQ
    paths = OQ.synth_bqsr_set(str(tmp_path), **B.FIXTURE)
    reads, rgs, _ = B.load(paths['sam'])
    cls, t = U.classes(reads, 15)
    got, info = U.vectors(reads, rgs, 15, classified=(cls, t))
    ones, _ = B.vectors(reads, rgs, 15, flagged=(cls == 1, t))
    twos, _ = B.vectors(reads, rgs, 15, flagged=(cls == 2, t))
    assert np.array_equal(cls == 1, B.flags(reads, 15)[0])
    assert info['flagged_bases'] == int((cls == 1).sum()) and info['skipped_bases'] == int((cls == 2).sum()) >= 50
    assert int(twos[1].sum()) >= 50                      # the tally sees unresolved bases: the option changes this fixture's report
    for e, tot in ((1, 2), (3, 4), (5, 6), (7, 8)):
        assert np.array_equal(got[e], ones[e]), B.VEC[e]
        assert np.array_equal(got[tot], ones[tot] - twos[e]), B.VEC[tot]


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
        if kw.get('skip_unresolved'):
            kw['info'].update(skipped_bases=17)
        return _Report(seen)
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: 'opened:' + p)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', kmers)
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: seen.update(report=a) or _Report(seen))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the command then leaves the memory back end alone
    return seen


def test_argparse_skip_unresolved_reaches_the_k_mer_report(monkeypatch, capsys):
    from kbbq import main
    seen = _patched(monkeypatch)
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-k', '15', '--skip-unresolved', '-g', 'r.grp'])
    bam, kw = seen['kmers']
    kw.pop('info')
    assert bam == 'opened:x.bam' and seen['out'] == 'r.grp'
    assert kw == dict(k=15, min_count=None, slots=None, prefilter=False, filter_bits=4, use_oq=False, skip_unresolved=True)
    err = capsys.readouterr().err
    assert err == 'kbbq bqsr: k=15 min_count=7 reads=5 flagged_bases=11 skipped_bases=17\n'
    assert re.search(r'^kbbq bqsr: k=15 min_count=\d+ reads=\d+ flagged_bases=\d+ skipped_bases=\d+$', err, flags=re.M)
    # ... composes with the other options; the new field sits directly after flagged_bases
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '--skip-unresolved', '--min-count', '3', '--slots', '4096', '--prefilter', '-u',
               '-g', 'r2.grp'])
    kw = seen['kmers'][1]
    kw.pop('info')
    assert kw == dict(k=31, min_count=3, slots=4096, prefilter=True, filter_bits=4, use_oq=True, skip_unresolved=True)
    assert capsys.readouterr().err == ('kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11 skipped_bases=17 prefilter=1 '
                                       'admitted=13 slots=1024\n')
    # ... and without it the call and the line are what they were
    main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r3.grp'])
    kw = seen['kmers'][1]
    kw.pop('info')
    assert kw == dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, use_oq=False)
    assert capsys.readouterr().err == 'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11\n'


def test_argparse_skip_unresolved_only_with_kmers(monkeypatch, capsys):
    from kbbq import main
    seen = _patched(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--skip-unresolved'])
    assert exc.value.code == 2 and not seen
    assert '--skip-unresolved: only with --kmers' in capsys.readouterr().err


def test_the_keyword_reaches_the_covariates(monkeypatch):
    from kbbq.gatk import bqsr
    seen = {}
    monkeypatch.setattr(bqsr.utils, 'get_rg_to_pu', lambda bam: {'g0': 'unit0'})
    monkeypatch.setattr(bqsr, 'bam_to_kmer_covariates', lambda bam, **kw: seen.update(kw) or 'vectors')
    monkeypatch.setattr(bqsr, 'vectors_to_report', lambda *a: a)
    assert bqsr.bam_to_report_kmers('bam', k=15, skip_unresolved=True) == tuple('vectors') + (['unit0'],)
    assert seen['skip_unresolved'] is True and seen['k'] == 15
    bqsr.bam_to_report_kmers('bam', k=15)
    assert seen['skip_unresolved'] is False


# ---------------------------------------------------------------- the C ABI
def test_symbol_is_exported_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    assert hasattr(lib, 'kbbq_kmer_flag_ex_dev')
    _vp, _i = N.PROTOTYPES['kbbq_kmer_flag_dev'][1][0], N.PROTOTYPES['kbbq_kmer_flag_dev'][0]
    assert N.PROTOTYPES['kbbq_kmer_flag_ex_dev'] == (_i, N.PROTOTYPES['kbbq_kmer_flag_dev'][1] + [_vp, _i])
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    assert 'int kbbq_kmer_flag_ex_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,' in header
    assert re.search(r'^#define KBBQ_KMER_FLAG_UNRESOLVED 2$', header, flags=re.M) and N.KMER_FLAG_UNRESOLVED == 2
    assert N.KMER_FLAG_UNRESOLVED & N.KMER_FIX_N == 0    # one option word


def test_device_free_refusals_of_the_call():
    """No context and no table exist without a device: every refusal below is decided on the arguments alone."""
    from kbbq import _native as N
    lib = N.load()
    for opts in (N.KMER_FIX_N, N.KMER_FIX_N | N.KMER_FLAG_UNRESOLVED, 4, 0x100):
        assert lib.kbbq_kmer_flag_ex_dev(None, None, None, None, 0, 16, 2, None, None, None, opts) == N.KBBQ_E_ARG
        assert 'kbbq_kmer_flag_ex_dev' in N.last_error() and 'opts' in N.last_error()
    for opts in (0, N.KMER_FLAG_UNRESOLVED):
        assert lib.kbbq_kmer_flag_ex_dev(None, None, None, None, 0, 16, 2, None, None, None, opts) == N.KBBQ_E_ARG
        assert 'NULL ctx or table' in N.last_error()
        assert lib.kbbq_kmer_flag_ex_dev(None, None, None, None, 1, 17, 2, None, None, None, opts) == N.KBBQ_E_ARG
        assert 'pitch must be a positive multiple of 16' in N.last_error()
        assert lib.kbbq_kmer_flag_ex_dev(None, None, None, None, 1, 16, 0, None, None, None, opts) == N.KBBQ_E_ARG
        assert 'min_count must be >= 1' in N.last_error()
