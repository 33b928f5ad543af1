"""kbbq_kmer_flag_ex_dev with KBBQ_KMER_FLAG_UNRESOLVED, kbbq.kmer.flag_errors(unresolved=True) and `kbbq bqsr --kmers
--skip-unresolved` on the MI355X: the flag plane with its third value against the CPU model (tests/kmer_unresolved_model.py) bit
for bit, the shapes at which the kernel takes another path, the nine vectors with the unresolved bases left out of the tally
(fused and unfused), and the command line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmer_bqsr_model as B
import kmer_model as M
import kmer_unresolved_model as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED'):
    ENV.pop(_var, None)

_memo = {}


def _device(x):
    import torch
    x = np.array(x)                                      # a writable copy: the shared inputs are read-only
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def _host(t):
    return t.cpu().numpy()


def _flag_ex(table, dseq, dmeta, t, opts, fill=0xAA, counts=True):
    """kbbq_kmer_flag_ex_dev into a plane and counters pre-filled with junk: (rc, the whole plane, changed, unresolved)."""
    import torch
    from kbbq import _native as N
    n, pitch = dseq.shape
    plane = torch.full((max(n, 1), pitch), fill, dtype=torch.uint8, device='cuda')
    changed = torch.full((max(n, 1),), -1, dtype=torch.int32, device='cuda')
    unres = torch.full((max(n, 1),), -1, dtype=torch.int32, device='cuda')
    rc = N.load().kbbq_kmer_flag_ex_dev(table.ctx.handle, table.handle, N.ptr(dseq), N.ptr(dmeta), n, pitch, int(t), N.ptr(plane),
                                        N.ptr(changed) if counts else None, N.ptr(unres) if counts else None, opts)
    if rc == N.KBBQ_OK:
        table.ctx.status()
    return rc, _host(plane[:n]), _host(changed[:n]).astype(np.int64), _host(unres[:n]).astype(np.int64)


# ---------------------------------------------------------------- 1. the flag plane against the model
def _reads():
    if 'reads' not in _memo:
        seq, meta = M.synth(5, genome_len=20000, depth=30, err=0.03, len_lo=36, len_hi=300)[:2]
        seq.setflags(write=False); meta.setflags(write=False)
        _memo['reads'] = (seq, meta)
    return _memo['reads']


def _model(k):
    """The model's classes of the read set for k (threshold from the histogram), computed once and left unchanged."""
    if k not in _memo:
        seq, meta = _reads()
        cls, ones, twos, t = U.classify(seq, meta, k)
        for a in (cls, ones, twos):
            a.setflags(write=False)
        _memo[k] = (cls, ones, twos, t)
    return _memo[k]


@pytest.mark.parametrize('k', [15, 21, 31])
def test_plane_equals_the_model_bit_for_bit(k):
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = _reads()
    want, ones, twos, t = _model(k)
    # the input holds the classes under test -- else this test would pass on nothing
    assert int((want == 1).sum()) >= 50 and int((want == 2).sum()) >= 50
    assert set(np.unique(want).tolist()) == {0, 1, 2}
    dseq, dmeta = _device(seq), _device(meta)
    table = kmer.count_kmers(dseq, dmeta, k=k)
    try:
        assert kmer.solid_threshold(kmer.kmer_histogram(table)) == t
        flags, changed, unres = kmer.flag_errors(table, dseq, dmeta, t, unresolved=True)
        assert flags.is_cuda and changed.is_cuda and unres.is_cuda and flags.shape == dseq.shape and flags.dtype == dseq.dtype
        got = _host(flags)
        assert np.array_equal(got, want)                                 # padding included
        assert np.array_equal(_host(changed).astype(np.int64), ones)
        assert np.array_equal(_host(unres).astype(np.int64), twos)
        # every byte is written, whatever the plane held; the counters may be NULL
        rc, plane, pchanged, punres = _flag_ex(table, dseq, dmeta, t, N.KMER_FLAG_UNRESOLVED)
        assert rc == N.KBBQ_OK and np.array_equal(plane, want) and np.array_equal(pchanged, ones) and np.array_equal(punres, twos)
        rc, plane, _, _ = _flag_ex(table, dseq, dmeta, t, N.KMER_FLAG_UNRESOLVED, counts=False)
        assert rc == N.KBBQ_OK and np.array_equal(plane, want)
        # without the option: the same plane with every 2 turned to 0 -- kbbq_kmer_flag_dev's, and opts = 0's
        plain, pchanged0 = kmer.flag_errors(table, dseq, dmeta, t)
        assert np.array_equal(_host(plain), np.where(want == 2, 0, want))
        assert np.array_equal(_host(pchanged0).astype(np.int64), ones)
        rc, plane, pchanged, punres = _flag_ex(table, dseq, dmeta, t, 0)
        assert rc == N.KBBQ_OK and np.array_equal(plane, _host(plain)) and np.array_equal(pchanged, ones) and not punres.any()
    finally:
        table.close()


# ---------------------------------------------------------------- 2. shapes where the kernel can go wrong
EDGE_K = 21
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b'ACGT')] = list(b'TGCA')


@pytest.fixture(scope='module')
def edge_table():
    """A table of error-free 100-base reads of a 6 kb genome at 20x (k = 21) that the rows below are judged against at
    min_count 3; their own k-mers are not in it.  (table, genome, the solid keys by the model's count)."""
    from kbbq import kmer
    seq, meta, genome, solid = _edge_reads()
    table = kmer.count_kmers(_device(seq), _device(meta), k=EDGE_K)
    yield table, genome, solid
    table.close()


def _edge_reads():
    rng = np.random.default_rng(21)
    genome = np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, 6000)]
    reads = []
    for _ in range(6000 * 20 // 100):
        s = int(rng.integers(0, 6000 - 100 + 1))
        x = genome[s:s + 100]
        reads.append((COMP[x][::-1] if rng.random() < 0.5 else x).tobytes())
    seq, meta = M.plane(reads)
    keys, counts = M.count(seq, meta, EDGE_K)
    return seq, meta, genome, keys[counts >= 3]


def _piece(genome, start, L, subs=(), ns=()):
    x = bytearray(genome[start:start + L].tobytes())
    for at in subs:
        x[at] = b'ACGT'[(b'ACGT'.index(x[at]) + 1) % 4]
    for at in ns:
        x[at] = ord('N')
    return bytes(x)


def _check(edge_table, reads, pitch=None):
    from kbbq import _native as N
    table, _, solid = edge_table
    seq, meta = M.plane(reads, pitch)
    want, ones, twos, _ = U.classify(seq, meta, EDGE_K, 3, solid_keys=solid)
    rc, plane, changed, unres = _flag_ex(table, _device(seq), _device(meta), 3, N.KMER_FLAG_UNRESOLVED)
    assert rc == N.KBBQ_OK
    assert np.array_equal(plane, want)
    assert np.array_equal(changed, ones) and np.array_equal(unres, twos)
    rc, plain, changed0, unres0 = _flag_ex(table, _device(seq), _device(meta), 3, 0)
    assert rc == N.KBBQ_OK and np.array_equal(plain, np.where(want == 2, 0, want)) and np.array_equal(changed0, ones) and not unres0.any()
    return want


def _short_rows(g):
    k = EDGE_K
    return [
        _piece(g, 100, 37, subs=(16, 20)),               # partial last chunk; each of the windows 0..16 holds both errors
        _piece(g, 200, 50, subs=(20,)),                  # one error in a short read: an error among unresolved bases
        _piece(g, 300, 99, subs=(40, 47, 54)),           # three errors within k bases: the middle one has no window of its own
        _piece(g, 400, k, subs=(10,)),                   # exactly k: one window
        _piece(g, 500, k, subs=(0, k - 1)),
        _piece(g, 600, k),
        _piece(g, 700, k - 1, subs=(10,)),               # k - 1: no window, all 0
        _piece(g, 800, 70, subs=(k - 1,), ns=(k,)),      # an error beside an N: window 0 is its only one
        _piece(g, 900, 70, subs=(12, k - 1), ns=(k,)),   # ... and unresolved beside an N
        _piece(g, 1000, 70, subs=(k + 1, k + 8), ns=(k,)),   # ... on the N's other side
        _piece(g, 1100, 97),                             # clean
        b'N' * 33,
    ]


def _short_rows_by_construction(want):
    k = EDGE_K
    assert want[0, :37].tolist() == [2] * 37
    assert want[1, :50].tolist() == [2] * 20 + [1] + [0] * 29        # the windows 21..29 are clean and cover the bases behind
    assert want[2, 47] == 2 and want[2, 40] == 1 and want[2, 54] == 1
    assert want[3, :k].tolist() == [2] * 10 + [1] + [2] * 10 and want[4, :k].tolist() == [2] * k
    assert not want[5].any() and not want[6].any() and not want[10].any() and not want[11].any()
    assert want[7, :k + 1].tolist() == [2] * (k - 1) + [1, 0] and not want[7, k + 1:].any()
    assert want[8, :k + 1].tolist() == [2] * k + [0] and not want[8, k + 1:].any()
    assert want[9, k] == 0 and want[9, k + 1] == 2 and not want[9, :k].any()


def test_short_rows_partial_chunks_and_a_wide_pitch(edge_table):
    """One plane, pitch 160 where 112 would do: lengths that are no multiple of 16, reads of exactly k and of k - 1 bases, a
    triple of errors within k bases, and unresolved bases on either side of an N."""
    reads = _short_rows(edge_table[1])
    want = _check(edge_table, reads, pitch=160)
    assert want.shape == (len(reads), 160)
    _short_rows_by_construction(want)
    # the same rows at the pitch they need: the same classes
    narrow = _check(edge_table, reads)
    assert narrow.shape[1] == 112 and np.array_equal(narrow, want[:, :112])


def test_one_row_of_more_than_256_chunks(edge_table):
    """4,100 bases: pitch 4,112, 257 chunks, one row a workgroup and thread 0 takes chunks 0 and 256.  Errors that leave
    unresolved bases on both sides of a chunk boundary (1,600) and of the 256-chunk stride (4,096)."""
    want = _check(edge_table, _long_rows(edge_table[1]))
    assert want.shape[1] == 4112 and want.shape[1] // 16 > 256
    _long_rows_by_construction(want)


def _long_rows(g):
    subs = (700, 1594, 1601, 1608, 2500, 2505, 4090, 4097)
    return [_piece(g, 50, 4100, subs=subs, ns=(3000,)), _piece(g, 200, 150, subs=(70, 80, 90))]


def _long_rows_by_construction(want):
    row = want[0]
    assert row[700] == 1 and row[1601] == 2 and row[4097] == 2 and row[4090] == 1
    assert (row[1590:1600] == 2).any() and (row[1600:1610] == 2).any()
    assert (row[4086:4096] == 2).any() and (row[4096:4100] == 2).any()
    assert not row[4100:].any() and row[3000] == 0


def test_no_reads_is_a_no_op(edge_table):
    import torch
    from kbbq import _native as N
    from kbbq import kmer
    table = edge_table[0]
    lib = N.load()
    plane = torch.full((1, 64), 0xAA, dtype=torch.uint8, device='cuda')
    for opts in (0, N.KMER_FLAG_UNRESOLVED):
        assert lib.kbbq_kmer_flag_ex_dev(table.ctx.handle, table.handle, None, None, 0, 64, 3, None, None, None, opts) == N.KBBQ_OK
        assert lib.kbbq_kmer_flag_ex_dev(table.ctx.handle, table.handle, N.ptr(plane), N.ptr(plane), 0, 64, 3, N.ptr(plane),
                                         N.ptr(plane), N.ptr(plane), opts) == N.KBBQ_OK
    table.ctx.status()
    assert int((plane != 0xAA).sum()) == 0
    flags, changed, unres = kmer.flag_errors(table, plane[:0], torch.zeros(0, dtype=torch.int32, device='cuda'), 3, unresolved=True)
    assert tuple(flags.shape) == (0, 64) and tuple(changed.shape) == (0,) and tuple(unres.shape) == (0,)


def test_refused_options_leave_the_context_usable(edge_table):
    from kbbq import _native as N
    table, g, _ = edge_table
    seq, meta = M.plane([_piece(g, 100, 37, subs=(16, 20))])
    dseq, dmeta = _device(seq), _device(meta)
    for opts in (N.KMER_FIX_N, N.KMER_FIX_N | N.KMER_FLAG_UNRESOLVED, 4, 0x40 | N.KMER_FLAG_UNRESOLVED):
        rc, plane, changed, unres = _flag_ex(table, dseq, dmeta, 3, opts)
        assert rc == N.KBBQ_E_ARG and 'opts' in N.last_error(), opts
        assert (plane == 0xAA).all() and (changed == -1).all() and (unres == -1).all()      # nothing was launched
    table.ctx.status()
    rc, plane, changed, unres = _flag_ex(table, dseq, dmeta, 3, N.KMER_FLAG_UNRESOLVED)
    assert rc == N.KBBQ_OK and plane[0, :37].tolist() == [2] * 37 and not plane[0, 37:].any()
    assert changed.tolist() == [0] and unres.tolist() == [37]


# ---------------------------------------------------------------- 3. the nine vectors
@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    """The alignments of tests/test_gpu_bqsr_kmers.py: both strands, read 2, soft clips, indels, three read groups."""
    import bamwriter
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('bqsr_kmers_unresolved')
    paths = OQ.synth_bqsr_set(str(d), **B.FIXTURE)
    paths['bam'] = str(bamwriter.write_bam(d / 'aln.bam', open(paths['sam']).read()))
    reads, rgs, pus = B.load(paths['sam'])
    assert len(reads) == 600 and len(rgs) == 3
    assert any(r.is_reverse for r in reads) and any(r.is_read2 for r in reads)
    assert any(op == 4 for r in reads for op, _ in r.cigartuples)
    return dict(paths=paths, reads=reads, rgs=rgs, pus=pus, dir=d)


def _want(fixture, k, t, use_oq):
    """(the model's vectors with the option, without it, info), computed once per (k, min_count, use_oq) and left unchanged."""
    memo = ('vectors', k, t, use_oq)
    if memo not in _memo:
        if ('classes', k, t) not in _memo:
            _memo[('classes', k, t)] = U.classes(fixture['reads'], k, t)
        cls, tt = _memo[('classes', k, t)]
        vec, info = U.vectors(fixture['reads'], fixture['rgs'], k, use_oq=use_oq, classified=(cls, tt))
        plain, _ = B.vectors(fixture['reads'], fixture['rgs'], k, use_oq=use_oq, flagged=(cls == 1, tt))
        for a in vec + plain:
            a.setflags(write=False)
        _memo[memo] = (vec, plain, info)
    vec, plain, info = _memo[memo]
    assert info['flagged_bases'] >= 50 and info['skipped_bases'] >= 50
    return vec, plain, info


def _same(got, want, what=''):
    assert len(got) == 9
    for name, g, w in zip(B.VEC, got, want):
        assert np.array_equal(g, w), (name, what)


CASES = [dict(k=15, min_count=None), dict(k=21, min_count=3, prefilter=True, use_oq=True)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join('%s=%s' % kv for kv in c.items()))
@pytest.mark.parametrize('fused', [None, '0'])
def test_vectors_leave_the_unresolved_bases_out(fixture, case, fused, monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    if fused is None:
        monkeypatch.delenv('KBBQ_TALLY_FUSED', raising=False)
    else:
        monkeypatch.setenv('KBBQ_TALLY_FUSED', fused)
    want, plain, winfo = _want(fixture, case['k'], case['min_count'], case.get('use_oq', False))
    # the option changes this fixture's tally: fewer observations, the same errors
    assert int(want[2].sum()) <= int(plain[2].sum()) - 50 and np.array_equal(want[1], plain[1])
    info = {}
    source = 'sam' if fused is None else 'bam'
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths'][source]), info=info, skip_unresolved=True, **case)
    _same(got, want, (case, fused))
    assert got[0].dtype == np.int64
    assert any(not np.array_equal(g, p) for g, p in zip(got, plain))
    assert not np.array_equal(got[2], plain[2]) and not np.array_equal(got[6], plain[6])
    assert info['k'] == case['k'] and info['min_count'] == winfo['min_count'] and info['reads'] == 600
    assert info['flagged_bases'] == winfo['flagged_bases'] and info['skipped_bases'] == winfo['skipped_bases']
    # ... and without it the vectors and `info` are what they were
    info0 = {}
    _same(bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths'][source]), info=info0, **case), plain, (case, fused, 'plain'))
    assert 'skipped_bases' not in info0 and info0['flagged_bases'] == winfo['flagged_bases']


# ---------------------------------------------------------------- 4. the command line
def _kbbq(*argv, timeout=300):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=ENV)


def _lines(r):
    return [ln for ln in r.stderr.decode().split('\n') if ln.startswith('kbbq bqsr:')]


def test_command_line(fixture, tmp_path):
    from kbbq import aln
    from kbbq.gatk import bqsr
    sam = fixture['paths']['sam']
    want, plain, winfo = _want(fixture, 15, None, False)
    wanted, wanted_plain = tmp_path / 'want.grp', tmp_path / 'want_plain.grp'
    bqsr.bam_to_report_kmers(aln.AlignmentFile(sam), k=15, skip_unresolved=True).write(str(wanted))
    bqsr.bam_to_report_kmers(aln.AlignmentFile(sam), k=15).write(str(wanted_plain))
    model = tmp_path / 'model.grp'
    bqsr.vectors_to_report(*want, fixture['pus']).write(str(model))
    assert wanted.read_bytes() == model.read_bytes() and wanted.read_bytes() != wanted_plain.read_bytes()
    grp = tmp_path / 'skip.grp'
    r = _kbbq('bqsr', '-b', sam, '--kmers', '-k', '15', '--skip-unresolved', '-g', str(grp))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == b'' and grp.read_bytes() == wanted.read_bytes()
    assert re.search(r'^kbbq bqsr: k=15 min_count=\d+ reads=\d+ flagged_bases=\d+ skipped_bases=\d+$', r.stderr.decode(), flags=re.M)
    line = 'kbbq bqsr: k=15 min_count=%d reads=600 flagged_bases=%d skipped_bases=%d' % (
        winfo['min_count'], winfo['flagged_bases'], winfo['skipped_bases'])
    assert _lines(r) == [line]
    # ... with the prefilter: the same report, the longer line
    grp2 = tmp_path / 'skip_pf.grp'
    r = _kbbq('bqsr', '-b', fixture['paths']['bam'], '--kmers', '-k', '15', '--skip-unresolved', '--prefilter', '-g', str(grp2))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert grp2.read_bytes() == wanted.read_bytes()
    assert re.search(r'^%s prefilter=1 admitted=\d+ slots=\d+$' % re.escape(line), r.stderr.decode(), flags=re.M)
    # ... without the flag: the report and the line of before
    grp3 = tmp_path / 'plain.grp'
    r = _kbbq('bqsr', '-b', sam, '--kmers', '-k', '15', '-g', str(grp3))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert grp3.read_bytes() == wanted_plain.read_bytes()
    assert _lines(r) == ['kbbq bqsr: k=15 min_count=%d reads=600 flagged_bases=%d' % (winfo['min_count'], winfo['flagged_bases'])]
    # ... and without --kmers the option is refused
    r = _kbbq('bqsr', '-b', sam, '-r', fixture['paths']['fa'], '-v', fixture['paths']['vcf'], '--skip-unresolved', '-g', str(tmp_path / 'no.grp'))
    assert r.returncode == 2 and b'--skip-unresolved: only with --kmers' in r.stderr and not (tmp_path / 'no.grp').exists()
    # applybqsr finishes the job with the code as it is
    out = tmp_path / 'recal.sam'
    r = _kbbq('applybqsr', '-b', sam, '-g', str(grp), '-o', str(out))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    before = [ln.split('\t') for ln in open(sam).read().split('\n') if ln and not ln.startswith('@')]
    after = [ln.split('\t') for ln in out.read_text().split('\n') if ln and not ln.startswith('@')]
    assert len(after) == len(before) == 600
    assert all(a[:10] + a[11:] == b[:10] + b[11:] for a, b in zip(after, before))
    assert sum(a[10] != b[10] for a, b in zip(after, before)) >= 1
    assert all(len(a[10]) == len(b[10]) for a, b in zip(after, before))
