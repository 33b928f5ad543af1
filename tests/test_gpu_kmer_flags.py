"""kbbq_kmer_flag_dev / kbbq.kmer.flag_errors on the MI355X: the correction's decision as a flag plane, against the CPU model
(tests/kmer_model.py) and against the plane the correction kernel itself writes -- the rule on the read set of
tests/test_gpu_kmer.py, the edges of a row, rows of more than 256 chunks, a prefiltered table and the call's refusals."""
import numpy as np
import pytest

import kmer_model as M

pytestmark = pytest.mark.gpu

_memo = {}


def _reads():
    if 'reads' not in _memo:
        seq, meta = M.synth(7, genome_len=20000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
        seq.setflags(write=False); meta.setflags(write=False)
        _memo['reads'] = (seq, meta)
    return _memo['reads']


def _model(k):
    """The model's answer on the read set for k, computed once and left unchanged."""
    if k not in _memo:
        seq, meta = _reads()
        out, changed, t = M.correct(seq, meta, k)
        flags = (out != seq).astype(np.uint8)
        flags.setflags(write=False); changed.setflags(write=False)
        _memo[k] = (flags, changed, t)
    return _memo[k]


def _device(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def _flag_into(table, dseq, dmeta, t, fill=0xAA):
    """kbbq_kmer_flag_dev into a plane pre-filled with `fill`: (the whole plane, changed)."""
    import torch
    from kbbq import _native as N
    n, pitch = dseq.shape
    plane = torch.full((max(n, 1), pitch), fill, dtype=torch.uint8, device='cuda')
    changed = torch.full((max(n, 1),), -1, dtype=torch.int32, device='cuda')
    N.check(N.load().kbbq_kmer_flag_dev(table.ctx.handle, table.handle, N.ptr(dseq), N.ptr(dmeta), n, pitch, int(t), N.ptr(plane),
                                        N.ptr(changed)))
    table.ctx.status()
    return plane[:n].cpu().numpy(), changed[:n].cpu().numpy().astype(np.int64)


@pytest.mark.parametrize('k', [21, 31])
def test_flags_equal_the_model_and_the_correction_kernel(k):
    from kbbq import kmer
    seq, meta = _reads()
    want, want_changed, t = _model(k)
    assert 1000 < int(want.sum()) < 0.05 * seq.size
    dseq, dmeta = _device(seq), _device(meta)
    table = kmer.count_kmers(dseq, dmeta, k=k)
    try:
        assert kmer.solid_threshold(kmer.kmer_histogram(table)) == t
        flags, changed = kmer.flag_errors(table, dseq, dmeta, t)
        assert flags.is_cuda and changed.is_cuda and flags.shape == dseq.shape and flags.dtype == dseq.dtype
        got = flags.cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(changed.cpu().numpy().astype(np.int64), want_changed)
        out, cchanged = kmer.correct_with(table, dseq, dmeta, t)
        assert np.array_equal(got, (out.cpu().numpy() != seq).astype(np.uint8))
        assert np.array_equal(changed.cpu().numpy(), cchanged.cpu().numpy())
        # every byte is written, padding included: nothing of the plane's earlier content survives
        plane, pchanged = _flag_into(table, dseq, dmeta, t)
        assert set(np.unique(plane).tolist()) <= {0, 1} and np.array_equal(plane, want) and np.array_equal(pchanged, want_changed)
        # d_changed may be NULL
        import torch
        from kbbq import _native as N
        again = torch.full(dseq.shape, 0xAA, dtype=torch.uint8, device='cuda')
        N.check(N.load().kbbq_kmer_flag_dev(table.ctx.handle, table.handle, N.ptr(dseq), N.ptr(dmeta), seq.shape[0], seq.shape[1], t,
                                            N.ptr(again), None))
        table.ctx.status()
        assert np.array_equal(again.cpu().numpy(), want)
    finally:
        table.close()


def _genome_reads(seed, genome_len, depth, L, k):
    """Error-free reads of length L from both strands of a random genome, as byte strings, and the genome's letters."""
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, genome_len)]
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b'ACGT')] = list(b'TGCA')
    reads = []
    for _ in range(genome_len * depth // L):
        s = int(rng.integers(0, genome_len - L + 1))
        x = genome[s:s + L]
        reads.append((comp[x][::-1] if rng.random() < 0.5 else x).tobytes())
    return reads, genome


EDGE_K = 21


@pytest.fixture(scope='module')
def edge_table():
    """A table of a 3 kb genome at 30x (k = 21) that the edge cases below are judged against; their own k-mers are not in it."""
    from kbbq import kmer
    reads, genome = _genome_reads(21, 3000, 30, 100, EDGE_K)
    seq, meta = M.plane(reads)
    keys, counts = M.count(seq, meta, EDGE_K)
    table = kmer.count_kmers(_device(seq), _device(meta), k=EDGE_K)
    yield table, genome, keys[counts >= 3]
    table.close()


def _model_against(solid_keys, seq, meta, k):
    """kmer_model.correct's rule against a GIVEN set of solid keys (the rows' own k-mers are not counted): flags, changed."""
    saved = M.count
    M.count = lambda s, m, kk: (solid_keys, np.full(solid_keys.size, 1 << 20, dtype=np.int64))
    try:
        out, changed, _ = M.correct(seq, meta, k, 1)
    finally:
        M.count = saved
    return (out != seq).astype(np.uint8), changed


def _with_error(genome, start, L, at):
    x = bytearray(genome[start:start + L].tobytes())
    x[at] = b'ACGT'[(b'ACGT'.index(x[at]) + 1) % 4]
    return bytes(x)


@pytest.mark.parametrize('case', ['shorter_than_k', 'exactly_k', 'k_plus_1', 'chunk_edge', 'only_n', 'lower_case', 'one_read'])
def test_edges_of_a_row(edge_table, case):
    table, genome, solid = edge_table
    k = EDGE_K
    if case == 'shorter_than_k':
        reads = [_with_error(genome, 100 + i, L, L // 2) for i, L in enumerate((1, 8, 15, 16, 17, 20))]
    elif case == 'exactly_k':
        reads = [_with_error(genome, 200, k, at) for at in (0, 10, k - 1)] + [genome[200:200 + k].tobytes()]
    elif case == 'k_plus_1':
        reads = [_with_error(genome, 300, k + 1, at) for at in (0, 1, 11, k - 1, k)]
    elif case == 'chunk_edge':
        reads = [_with_error(genome, 400 + L, L, at) for L in (47, 48, 49) for at in (0, 15, 16, 31, 32, L - 2, L - 1)]
    elif case == 'only_n':
        reads = [b'N' * 60, _with_error(genome, 500, 60, 30)]
    elif case == 'lower_case':
        good = _with_error(genome, 600, 64, 40)
        reads = [good.lower(), good[:20] + good[20:24].lower() + good[24:], good]
    else:
        reads = [_with_error(genome, 700, 90, 45)]
    seq, meta = M.plane(reads)
    want, want_changed = _model_against(solid, seq, meta, k)
    plane, changed = _flag_into(table, _device(seq), _device(meta), 3)
    assert np.array_equal(plane, want), case
    assert np.array_equal(changed, want_changed)
    if case in ('shorter_than_k',):
        assert not want.any()                            # no window: all 0
    if case == 'only_n':
        assert not want[0].any() and want[1].sum() == 1
    if case in ('exactly_k', 'k_plus_1', 'chunk_edge', 'one_read'):
        assert want.sum() >= len(reads) - 1              # the planted errors are found (a tie may hide one)
    if case == 'lower_case':
        assert not want[0].any() and want[2].sum() == 1


def test_no_reads_is_a_no_op(edge_table):
    import torch
    from kbbq import _native as N
    from kbbq import kmer
    table = edge_table[0]
    plane = torch.full((1, 64), 0xAA, dtype=torch.uint8, device='cuda')
    assert N.load().kbbq_kmer_flag_dev(table.ctx.handle, table.handle, None, None, 0, 64, 3, None, None) == N.KBBQ_OK
    assert N.load().kbbq_kmer_flag_dev(table.ctx.handle, table.handle, N.ptr(plane), N.ptr(plane), 0, 64, 3, N.ptr(plane), None) == N.KBBQ_OK
    table.ctx.status()
    assert int((plane != 0xAA).sum()) == 0
    flags, changed = kmer.flag_errors(table, plane[:0], torch.zeros(0, dtype=torch.int32, device='cuda'), 3)
    assert tuple(flags.shape) == (0, 64) and tuple(changed.shape) == (0,)


def test_refusals_with_a_context(edge_table):
    import torch
    from kbbq import _native as N
    table = edge_table[0]
    lib, h, t = N.load(), table.ctx.handle, table.handle
    seq = torch.zeros((2, 64), dtype=torch.uint8, device='cuda')
    meta = torch.full((2,), 64, dtype=torch.int32, device='cuda')
    out = torch.zeros((2, 80), dtype=torch.uint8, device='cuda')
    args = lambda **kw: [kw.get('ctx', h), kw.get('table', t), kw.get('seq', N.ptr(seq)), kw.get('meta', N.ptr(meta)), 2,
                         kw.get('pitch', 64), kw.get('mc', 3), kw.get('out', N.ptr(out)), None]
    for kw, word in ((dict(pitch=60), 'pitch'), (dict(mc=0), 'min_count'), (dict(table=None), 'NULL'), (dict(ctx=None), 'NULL'),
                     (dict(seq=None), 'NULL'), (dict(meta=None), 'NULL'), (dict(out=None), 'NULL'),
                     (dict(out=N.ptr(out.view(-1)[8:])), 'aligned')):
        assert lib.kbbq_kmer_flag_dev(*args(**kw)) == N.KBBQ_E_ARG, kw
        assert word in N.last_error(), (kw, N.last_error())
    assert lib.kbbq_kmer_flag_dev(*args()) == N.KBBQ_OK
    table.ctx.status()


def test_rows_of_more_than_256_chunks():
    """3 reads of 4,100+ bases (pitch > 4096: one row a workgroup, every thread several chunks) from a 6 kb genome."""
    from kbbq import kmer
    rng = np.random.default_rng(9)
    k = 31
    short, genome = _genome_reads(31, 6000, 12, 150, k)
    long_ = []
    for i, L in enumerate((4100, 4113, 4500)):
        x = bytearray(genome[100 * i:100 * i + L].tobytes())
        for at in rng.choice(L, size=40, replace=False):
            x[at] = b'ACGT'[(b'ACGT'.index(x[at]) + int(rng.integers(1, 4))) % 4]
        x[2000 + i] = ord('N')
        long_.append(bytes(x))
    seq, meta = M.plane(long_)
    assert seq.shape[1] > 4096 and seq.shape[1] // 16 > 256
    sseq, smeta = M.plane(short)
    # the model counts one set of rows: the short reads padded to the long rows' pitch, then the long rows
    allseq = np.full((len(short) + 3, seq.shape[1]), ord('N'), dtype=np.uint8)
    allseq[:len(short), :sseq.shape[1]] = sseq
    allseq[len(short):] = seq
    allmeta = np.concatenate([smeta, meta])
    out, changed, _ = M.correct(allseq, allmeta, k, 2)
    want, want_changed = (out != allseq)[len(short):].astype(np.uint8), changed[len(short):]
    assert want.sum() >= 60
    dseq, dmeta = _device(seq), _device(meta)
    table = kmer.count_kmers(_device(sseq), _device(smeta), k=k)
    try:
        kmer.count_kmers(dseq, dmeta, table=table)
        plane, got_changed = _flag_into(table, dseq, dmeta, 2)
        assert np.array_equal(plane, want) and np.array_equal(got_changed, want_changed)
        out, _ = kmer.correct_with(table, dseq, dmeta, 2)
        assert np.array_equal(plane, (out.cpu().numpy() != seq).astype(np.uint8))
    finally:
        table.close()


def test_a_prefiltered_table_gives_the_same_flags():
    from kbbq import kmer
    seq, meta = _reads()
    k = 31
    want, want_changed, t = _model(k)
    dseq, dmeta = _device(seq), _device(meta)
    filt = kmer.prefilter_kmers(dseq, dmeta, k=k)
    filt.release_seen()
    table = kmer.count_kmers(dseq, dmeta, k=k, filter=filt)
    filt.close()
    try:
        for mc in sorted({2, t}):
            flags, changed = kmer.flag_errors(table, dseq, dmeta, mc)
            if mc == t:
                assert np.array_equal(flags.cpu().numpy(), want) and np.array_equal(changed.cpu().numpy().astype(np.int64), want_changed)
            else:
                out, _ = kmer.correct_with(table, dseq, dmeta, mc)
                assert np.array_equal(flags.cpu().numpy(), (out.cpu().numpy() != seq).astype(np.uint8))
                assert int(flags.sum()) > 1000
    finally:
        table.close()
