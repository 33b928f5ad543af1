"""`kbbq benchmark --kmers` on the MI355X: kbbq_flag_confusion_dev against NumPy on random planes (lengths, padding, skip bit,
class bits, offsets, adding, a hot bin, the error status, several launches), kbbq.benchmark.benchmark_kmers against the CPU model
(tests/kmer_benchmark_model.py) through SAM and BAM on records of one length and of mixed lengths, and the command line.  Every
count is an integer and every comparison exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmer_benchmark_model as KB
import kmer_bqsr_model as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS'):
    ENV.pop(_var, None)


# ---------------------------------------------------------------- the kernel against NumPy
def numpy_joint(qual, truth, kflags, lens, qoffset):
    """joint[q][bit 0 of truth][class] over the bases inside their reads whose bit 1 of truth is clear."""
    n, pitch = qual.shape
    counted = (np.arange(pitch)[None, :] < np.asarray(lens, dtype=np.int64)[:, None]) & ((truth & 2) == 0)
    q = qual.astype(np.int64) - qoffset
    assert (q[counted] >= 0).all()
    k = np.where(kflags & 1, 1, np.where(kflags & 2, 2, 0)).astype(np.int64)
    J = np.zeros((256, 2, 3), dtype=np.int64)
    np.add.at(J, (q[counted], (truth & 1).astype(np.int64)[counted], k[counted]), 1)
    return J


TRUTH_BYTES = np.array([0, 1, 2, 3, 0xFF, 0xFE, 0x82, 0x06], dtype=np.uint8)     # bit 1 set: skipped, whatever else is set
TRUTH_P = np.array([0.55, 0.2, 0.05, 0.04, 0.04, 0.04, 0.04, 0.04])
KFLAG_BYTES = np.array([0, 1, 2, 3], dtype=np.uint8)                             # 3: bit 0 wins, class 1
KFLAG_P = np.array([0.6, 0.15, 0.15, 0.1])


def random_planes(seed, lens, pitch, qoffset):
    """(qual, truth, kflags) with 0xFF at and beyond every length in all three planes."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.uint32)
    n = len(lens)
    qual = (rng.integers(0, 45, size=(n, pitch)) + qoffset).astype(np.uint8)
    truth = rng.choice(TRUTH_BYTES, size=(n, pitch), p=TRUTH_P)
    kflags = rng.choice(KFLAG_BYTES, size=(n, pitch), p=KFLAG_P)
    beyond = np.arange(pitch)[None, :] >= lens[:, None].astype(np.int64)
    for a in (qual, truth, kflags):
        a[beyond] = 0xFF
    return qual, truth, kflags


SHAPES = {
    'one-base': (np.array([1]), 16),
    'five-rows': (np.array([0, 1, 16, 17, 48]), 48),
    'many-rows': (np.random.default_rng(5).integers(0, 151, size=4099), 160),
}
_planes = {}


def planes(shape, qoffset):
    """The random planes of a shape, their NumPy answer and their device copies: made once, left unchanged."""
    import torch
    key = (shape, qoffset)
    if key not in _planes:
        lens, pitch = SHAPES[shape]
        host = random_planes(17 + len(lens), lens, pitch, qoffset)
        want = numpy_joint(*host, lens, qoffset)
        want.setflags(write=False)
        _planes[key] = dict(lens=lens.astype(np.uint32), pitch=pitch, host=host, want=want,
                            dev=tuple(torch.from_numpy(a).cuda() for a in host))
    return _planes[key]


def call(dev_planes, lens, pitch, qoffset, counts):
    """kbbq_flag_confusion_dev itself, then the context's status."""
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    d_len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).cuda()
    ctx = dev.context()
    q, t, k = dev_planes
    N.check(N.load().kbbq_flag_confusion_dev(ctx.handle, N.ptr(q), N.ptr(t), N.ptr(k), N.ptr(d_len), len(lens), pitch, qoffset,
                                             N.ptr(counts)))
    ctx.status()


@pytest.mark.parametrize('qoffset', [0, 33])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_kernel_against_numpy_on_random_planes(shape, qoffset):
    """The occupancy the issue asks of the input (all six [t][k] cells, at least 20 qualities) is asserted where the shape can
    hold it, the 4099 rows; one base and five rows are asserted to count something and to hold skipped bases and padding."""
    import torch
    from kbbq import benchmark
    p = planes(shape, qoffset)
    want, lens, pitch = p['want'], p['lens'], p['pitch']
    q, t, k = p['host']
    if shape == 'many-rows':
        assert (want.sum(axis=0) > 0).all() and int((want.sum(axis=(1, 2)) > 0).sum()) >= 20
        inside = np.arange(pitch)[None, :] < lens[:, None].astype(np.int64)
        assert (inside & np.isin(t, [0xFF, 0xFE, 0x82, 0x06])).any() and (inside & (t == 3)).any()     # skipped with other bits set
        assert (inside & (k == 3) & ((t & 2) == 0)).any() and int(want[:, :, 1].sum()) > int(((k == 1) & inside & ((t & 2) == 0)).sum())
        assert lens.min() == 0 and lens.max() == 150
    assert int(want.sum()) == int(((np.arange(pitch)[None, :] < lens[:, None].astype(np.int64)) & ((t & 2) == 0)).sum())
    assert all((a[np.arange(pitch)[None, :] >= lens[:, None].astype(np.int64)] == 0xFF).all() for a in (q, t, k))
    got = benchmark.kmer_confusion(*p['dev'], lens, pitch, qoffset)
    assert got.dtype == np.int64 and got.shape == (256, 2, 3)
    assert np.array_equal(got, want)
    # the call adds: counters pre-filled with junk keep it, a second call doubles the counts
    junk = np.random.default_rng(3).integers(-1 << 40, 1 << 40, size=1536)
    counts = torch.from_numpy(junk.copy()).cuda()
    call(p['dev'], lens, pitch, qoffset, counts)
    assert np.array_equal(counts.cpu().numpy(), junk + want.reshape(-1))
    call(p['dev'], lens, pitch, qoffset, counts)
    assert np.array_equal(counts.cpu().numpy(), junk + 2 * want.reshape(-1))


def test_no_rows_is_no_launch():
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import benchmark
    counts = torch.full((1536,), 7, dtype=torch.int64, device='cuda')
    assert N.load().kbbq_flag_confusion_dev(dev.context().handle, N.ptr(counts), N.ptr(counts), N.ptr(counts), N.ptr(counts), 0, 16, 33,
                                            N.ptr(counts)) == N.KBBQ_OK
    assert int(counts.sum().item()) == 7 * 1536
    empty = torch.zeros((1, 16), dtype=torch.uint8, device='cuda')
    assert not benchmark.kmer_confusion(empty, empty, empty, np.zeros(0, dtype=np.uint32), 16, 33).any()


def test_hot_bin():
    """4096 full rows of 256 bases into ONE bin: 1,048,576 increments (the 32-bit counters of a workgroup take all of its
    share); then the same total with the bytes alternating between two classes."""
    import torch
    from kbbq import benchmark
    n, pitch = 4096, 256
    lens = np.full(n, pitch, dtype=np.uint32)
    qual = torch.full((n, pitch), 33 + 40, dtype=torch.uint8, device='cuda')
    truth = torch.ones((n, pitch), dtype=torch.uint8, device='cuda')
    kflags = torch.ones((n, pitch), dtype=torch.uint8, device='cuda')
    got = benchmark.kmer_confusion(qual, truth, kflags, lens, pitch, 33)
    want = np.zeros((256, 2, 3), dtype=np.int64)
    want[40, 1, 1] = n * pitch
    assert n * pitch == 1048576 and np.array_equal(got, want)
    kflags = torch.from_numpy(np.tile(np.array([0, 2], dtype=np.uint8), (n, pitch // 2))).cuda()
    got = benchmark.kmer_confusion(qual, truth, kflags, lens, pitch, 33)
    want = np.zeros((256, 2, 3), dtype=np.int64)
    want[40, 1, 0] = want[40, 1, 2] = n * pitch // 2
    assert np.array_equal(got, want)


def _status_planes(truth_byte, length):
    """Nine rows of 32 bytes, quality 'S' everywhere but one byte below '!' at base 20 of read 6."""
    import torch
    n, pitch = 9, 32
    qual = np.full((n, pitch), ord('S'), dtype=np.uint8)
    qual[6, 20] = 10
    truth = np.zeros((n, pitch), dtype=np.uint8)
    truth[6, 20] = truth_byte
    kflags = np.zeros((n, pitch), dtype=np.uint8)
    lens = np.full(n, 32, dtype=np.uint32)
    lens[6] = length
    return tuple(torch.from_numpy(a).cuda() for a in (qual, truth, kflags)), lens, pitch


def test_error_status(monkeypatch):
    from kbbq import benchmark
    dev_planes, lens, pitch = _status_planes(0, 32)
    with pytest.raises(ValueError, match=r'read 6\b') as exc:
        benchmark.kmer_confusion(*dev_planes, lens, pitch, 33)
    assert exc.value.read_index == 6
    got = benchmark.kmer_confusion(*dev_planes, lens, pitch, 0)            # no offset: the byte is quality 10
    assert got[10, 0, 0] == 1 and got[ord('S'), 0, 0] == 9 * 32 - 1 and got.sum() == 9 * 32
    # ... in a later launch of several: still the read's own index
    monkeypatch.setattr(benchmark, 'CONFUSION_BASES_PER_LAUNCH', 4 * pitch)
    with pytest.raises(ValueError, match=r'read 6\b') as exc:
        benchmark.kmer_confusion(*dev_planes, lens, pitch, 33)
    assert exc.value.read_index == 6
    monkeypatch.undo()
    # the same byte at a skipped base, and beyond the length: nothing
    for truth_byte, length in ((2, 32), (3, 32), (0, 20), (0, 5)):
        dev_planes, lens, pitch = _status_planes(truth_byte, length)
        got = benchmark.kmer_confusion(*dev_planes, lens, pitch, 33)
        assert got.sum() == 8 * 32 + min(length, 32) - (1 if length > 20 else 0) and got[ord('S') - 33, 0, 0] == got.sum()


def test_several_launches_give_the_counts_of_one(monkeypatch):
    from kbbq import _native as N
    from kbbq import benchmark
    p = planes('many-rows', 33)
    lib = N.load()
    real, calls = lib.kbbq_flag_confusion_dev, []

    def counted(*a):
        calls.append(a[5])
        return real(*a)
    monkeypatch.setattr(lib, 'kbbq_flag_confusion_dev', counted)
    monkeypatch.setattr(benchmark, 'CONFUSION_BASES_PER_LAUNCH', 1000)
    got = benchmark.kmer_confusion(*p['dev'], p['lens'], p['pitch'], 33)
    assert np.array_equal(got, p['want'])
    assert len(calls) == -(-4099 // 6) and sum(calls) == 4099 and max(calls) * p['pitch'] <= 1000


# ---------------------------------------------------------------- benchmark_kmers against the model
_memo = {}


@pytest.fixture(scope='module')
def one_length(tmp_path_factory):
    """Fixture (a): 600 records of 60 bases."""
    import bamwriter
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('benchmark_kmers_a')
    paths = OQ.synth_bqsr_set(str(d), **B.FIXTURE)
    paths['bam'] = str(bamwriter.write_bam(d / 'aln.bam', open(paths['sam']).read()))
    return dict(paths=paths, name='a', dir=d)


@pytest.fixture(scope='module')
def mixed_lengths(tmp_path_factory):
    """Fixture (b): 2400 records of 36..158 bases with hard and soft clips."""
    import bamwriter
    import oracle_benchmark as OB
    d = tmp_path_factory.mktemp('benchmark_kmers_b')
    paths = OB.synth_truthset(str(d), 7, npairs=1200, contigs=(('chr1', 2500), ('chr2', 1500)))
    paths['bam'] = str(bamwriter.write_bam(d / 'aln.bam', open(paths['sam']).read()))
    return dict(paths=paths, name='b', dir=d)


def model(fx, k, t=None, use_oq=False, bed=False):
    """(joint, info) of the model, computed once per case and left unchanged."""
    import kmer_unresolved_model as U
    name = fx['name']
    if (name, 'files', bed) not in _memo:
        _memo[(name, 'files', bed)] = KB.load(fx['paths'], bed=bed)
    reads, ref, skips = _memo[(name, 'files', bed)]
    if (name, 'classes', k, t) not in _memo:               # the classes depend on neither the qualities nor the skips
        _memo[(name, 'classes', k, t)] = U.classes(reads, k, t)
    key = (name, k, t, use_oq, bed)
    if key not in _memo:
        J, info = KB.joint(reads, ref, skips, k, t, use_oq=use_oq, classified=_memo[(name, 'classes', k, t)])
        J.setflags(write=False)
        _memo[key] = (J, info)
    return _memo[key]


def product(fx, source, k, bed=False, **kw):
    from kbbq import aln, benchmark
    p = fx['paths']
    info = {}
    fh = open(p['bed']) if bed else None
    try:
        got = benchmark.benchmark_kmers(aln.AlignmentFile(p[source]), benchmark.get_ref_dict(p['fa']), benchmark.get_var_sites(p['vcf']),
                                        k=k, bedfh=fh, info=info, **kw)
    finally:
        if fh:
            fh.close()
    return got, info


def same_info(info, winfo, prefilter=False):
    for name in ('k', 'min_count', 'reads', 'bases', 'errors', 'flagged', 'flagged_errors', 'unresolved', 'unresolved_errors'):
        assert info[name] == winfo[name], name
    assert info['prefilter'] is prefilter and (info['admitted'] is not None) == prefilter and info['slots'] >= 1024


@pytest.mark.parametrize('use_oq', [False, True])
@pytest.mark.parametrize('k', [15, 21])
@pytest.mark.parametrize('source', ['sam', 'bam'])
def test_one_length_equals_the_model(one_length, source, k, use_oq):
    want, winfo = model(one_length, k, use_oq=use_oq)
    cells = want.sum(axis=0)
    assert cells.min() >= 50 and int((want.sum(axis=(1, 2)) > 0).sum()) >= 20, cells       # a degenerate fixture fails
    got, info = product(one_length, source, k, use_oq=use_oq)
    assert got.dtype == np.int64 and got.shape == (256, 2, 3)
    assert np.array_equal(got, want)
    assert winfo['reads'] == 600
    same_info(info, winfo)


@pytest.mark.parametrize('bed', [False, True])
@pytest.mark.parametrize('k', [15, 21])
@pytest.mark.parametrize('source', ['sam', 'bam'])
def test_mixed_lengths_equal_the_model(mixed_lengths, source, k, bed):
    want, winfo = model(mixed_lengths, k, bed=bed)
    reads = _memo[('b', 'files', bed)][0]
    lens = [len(r.query_sequence) for r in reads]
    assert len(reads) == 2400 and min(lens) < 40 and max(lens) > 150 and len(set(lens)) > 50
    assert any(op == 5 for r in reads for op, _ in r.cigartuples) and any(op == 4 for r in reads for op, _ in r.cigartuples)
    assert want.sum(axis=0).min() >= (1 if bed else 10), want.sum(axis=0)
    got, info = product(mixed_lengths, source, k, bed=bed)
    assert np.array_equal(got, want)
    same_info(info, winfo)


def test_prefilter_min_count_and_the_existing_path(mixed_lengths, one_length):
    from kbbq import aln, benchmark
    for fx, k in ((mixed_lengths, 15), (one_length, 21)):
        want, winfo = model(fx, k)
        got, info = product(fx, 'sam', k, prefilter=True)
        assert np.array_equal(got, want)
        same_info(info, winfo, prefilter=True)
        assert 0 < info['admitted']
        # min_count given is honoured (not the valley's)
        t = winfo['min_count'] + 2
        want_t, winfo_t = model(fx, k, t=t)
        assert not np.array_equal(want_t, want)
        for kw in (dict(), dict(prefilter=True)):
            got, info = product(fx, 'sam', k, min_count=t, **kw)
            assert np.array_equal(got, want_t) and info['min_count'] == t
            same_info(info, winfo_t, prefilter=bool(kw))
        # summed over the k-mer classes the array is what benchmark_bam counts on the same input
        p = fx['paths']
        ref, var = benchmark.get_ref_dict(p['fa']), benchmark.get_var_sites(p['vcf'])
        skips = benchmark.get_full_skips(ref, var)
        err, skip, lens, pitch = benchmark._flag_batch(aln.AlignmentFile(p['sam']), benchmark._Genome(ref, skips), flip_reverse=False,
                                                       fused=True)
        qual = benchmark._qual_chars_dev(aln.AlignmentFile(p['sam']), lens, pitch, False)
        numerrs, numtotal = benchmark._count_q(qual, err, skip, lens, pitch, 33)
        assert np.array_equal(want.sum(axis=(1, 2)), numtotal) and np.array_equal(want[:, 1, :].sum(axis=1), numerrs)
        actual_q, nbases = benchmark.benchmark_bam(aln.AlignmentFile(p['sam']), ref, var)
        assert np.array_equal(nbases, want.sum(axis=(1, 2))[:len(nbases)]) and not want.sum(axis=(1, 2))[len(nbases):].any()


def test_records_shorter_than_k_are_class_0(mixed_lengths):
    """Forty records as they are and the same forty cut to their first 20 bases, at k = 32: the short ones have no window, so
    all their bases are class 0 (the model agrees), and they are counted by quality and truth like any other."""
    p = mixed_lengths['paths']
    lines = open(p['sam']).read().split('\n')
    few = [ln for ln in lines if ln and not ln.startswith('@')][:40]
    cut = mixed_lengths['dir'] / 'cut.sam'
    # 40 whole records, and the same records cut to their first 20 bases (CIGAR 20M): no record of the second half has a window
    out = [ln for ln in lines if ln.startswith('@')] + few
    for ln in few:
        f = ln.split('\t')
        f[0], f[5], f[9], f[10] = f[0] + 's', '20M', f[9][:20], f[10][:20]
        out.append('\t'.join(x for x in f if not x.startswith('OQ:Z:')))
    cut.write_text('\n'.join(out) + '\n')
    fx = dict(paths=dict(p, sam=str(cut)), name='cut', dir=mixed_lengths['dir'])
    want, winfo = model(fx, 32, t=2)
    got, info = product(fx, 'sam', 32, min_count=2)
    assert np.array_equal(got, want)
    same_info(info, winfo)
    assert info['reads'] == 80 and info['bases'] > 0


def test_quality_checks_are_those_of_benchmark_bam(mixed_lengths):
    from kbbq import aln, benchmark
    p = mixed_lengths['paths']
    lines = open(p['sam']).read().split('\n')
    first = next(i for i, ln in enumerate(lines) if ln and not ln.startswith('@'))

    def edited(name, fn):
        out = list(lines)
        out[first + 4] = '\t'.join(fn(lines[first + 4].split('\t')))
        path = mixed_lengths['dir'] / name
        path.write_text('\n'.join(out))
        return dict(mixed_lengths, paths=dict(p, sam=str(path)))
    with pytest.raises(KeyError, match='OQ'):
        product(edited('no_oq.sam', lambda f: [x for x in f if not x.startswith('OQ:Z:')]), 'sam', 15, use_oq=True)
    with pytest.raises(IndexError, match='read 4 has'):
        product(edited('short_qual.sam', lambda f: f[:10] + [f[10][:-1]] + f[11:]), 'sam', 15)
    with pytest.raises(ValueError, match='qualities must lie in 0..255'):
        product(edited('low_qual.sam', lambda f: f[:10] + [' ' + f[10][1:]] + f[11:]), 'sam', 15)


# ---------------------------------------------------------------- the command line
def _kbbq(*argv, timeout=300):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=ENV)


def _summary(stderr):
    return [ln for ln in stderr.decode().split('\n') if ln.startswith('kbbq benchmark:')]


def test_command_line(one_length):
    p = one_length['paths']
    want, winfo = model(one_length, 15)
    base = ('benchmark', '-b', p['sam'], '-r', p['fa'], '-v', p['vcf'])
    r = _kbbq(*base, '--kmers', '-k', '15', '-l', 'lbl')
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == KB.render(want, 'lbl')
    assert _summary(r.stderr) == [KB.summary(winfo)]
    # without --kmers: what it printed before, which is four columns of the new table
    old = _kbbq(*base, '-l', 'lbl')
    assert old.returncode == 0, old.stderr.decode()[-3000:]
    assert b'kbbq benchmark:' not in old.stderr
    import _shim
    import oracle_benchmark as OB
    oref = OB.get_ref_dict(p['fa'])
    rows = [ln.split('\t') for ln in r.stdout.decode().split('\n')[1:] if ln]
    assert old.stdout.decode() == ''.join('%s\t%s\t%s\t%s\n' % (f[0], f[7], f[10], f[1]) for f in rows)
    actual_q, nbases = OB.benchmark_bam(list(_shim.AlignmentFile(p['sam'])), oref, OB.get_var_sites(p['vcf']))
    assert old.stdout.decode() == OB.format_benchmark(actual_q, 'lbl', nbases)


def test_command_line_with_oq_and_with_the_prefilter(one_length):
    p = one_length['paths']
    want, winfo = model(one_length, 15)
    base = ('benchmark', '-b', p['sam'], '-r', p['fa'], '-v', p['vcf'])
    # the label defaults to the file, as for benchmark -b
    r = _kbbq(*base, '--kmers', '-k', '15', '-u', '--min-count', '3')
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    want_u, winfo_u = model(one_length, 15, t=3, use_oq=True)
    assert r.stdout.decode() == KB.render(want_u, p['sam']) and _summary(r.stderr) == [KB.summary(winfo_u)]
    r = _kbbq('benchmark', '-b', p['bam'], '-r', p['fa'], '-v', p['vcf'], '--kmers', '-k', '15', '--prefilter', '-l', 'lbl')
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == KB.render(want, 'lbl')
    line = _summary(r.stderr)
    assert len(line) == 1 and re.fullmatch(re.escape(KB.summary(winfo)) + r' prefilter=1 admitted=\d+ slots=\d+', line[0])
