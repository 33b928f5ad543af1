"""`--passes P` on the MI355X: km_correct_passes through the four kbbq_kmer_*_passes* calls, kbbq.kmer's `passes` keyword and the
four commands, against the CPU model of the repeated rule (tests/kmer_passes_model.py) byte for byte -- hand-built rows whose
passes are known by construction at the pitches where the kernel's geometry changes, a mixed-length set (13 rows a workgroup,
the last workgroup partial), one row of more than 256 chunks, the N rule, 4-bit planes and pair rows -- and, without the model,
against the one-pass kernel applied P times by hand."""
import glob
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M
import kmer_passes_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED'):
    ENV.pop(_var, None)
RANKS = 3
SECOND = np.uint32(1 << 31)

_memo = {}


def _device(x):
    import torch
    x = np.array(x)                                      # a writable copy: the shared inputs are read-only
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def _host(t):
    return t.cpu().numpy()


def _frozen(steps):
    for step in steps:
        for a in step:
            a.setflags(write=False)
    return steps


def _all_forms(table, seq, meta, t, P, want, fix_n=False):
    """The corrected form from device and from host buffers and the flag form with and without its 2s, each against `want` =
    (plane, changed, flags, ran) of the model."""
    from kbbq import kmer
    plane, changed, flags, _ = want
    dseq, dmeta = _device(seq), _device(meta)
    out, ch = kmer.correct_with(table, dseq, dmeta, t, fix_n=fix_n, passes=P)
    assert out.is_cuda and np.array_equal(_host(out), plane), P
    assert np.array_equal(_host(ch).astype(np.int64), changed), P
    out, ch = kmer.correct_with(table, seq, meta, t, fix_n=fix_n, passes=P)
    assert isinstance(out, np.ndarray) and np.array_equal(out, plane) and np.array_equal(ch.astype(np.int64), changed), P
    if fix_n:                                            # the flag form has no N rule
        return
    fl, ch, un = kmer.flag_errors(table, dseq, dmeta, t, unresolved=True, passes=P)
    assert np.array_equal(_host(fl), flags), P           # padding included; no byte is 3
    assert np.array_equal(_host(ch).astype(np.int64), (flags == 1).sum(axis=1)) and np.array_equal(_host(ch).astype(np.int64), changed)
    assert np.array_equal(_host(un).astype(np.int64), (flags == 2).sum(axis=1))
    fl, ch = kmer.flag_errors(table, dseq, dmeta, t, passes=P)
    assert np.array_equal(_host(fl), np.where(flags == 2, 0, flags)) and np.array_equal(_host(ch).astype(np.int64), changed), P
    assert np.array_equal(_host(dseq), seq)              # the input plane is as it was


# ---------------------------------------------------------------- 1. hand-built rows
@pytest.mark.parametrize('pitch, cut', ((16, PM.HAND_K - 1), (16, 16), (48, None), (64, None)))
def test_hand_built_rows(pitch, cut):
    from kbbq import kmer
    seq, meta, cases = PM.hand_rows(pitch=pitch, cut=cut)
    assert seq.shape[1] == pitch
    steps = PM.trace(seq, meta, PM.HAND_K, PM.HAND_T, 8)
    if cut is None:                                      # the rows need their passes: the comparison below cannot pass on nothing
        sums = [int(s[1].sum()) for s in steps]
        assert sums[0] < sums[1] < sums[2] == sums[7]
        assert not np.array_equal(steps[1][2], steps[2][2]) and not np.array_equal(steps[2][2], steps[3][2])
    elif cut < PM.HAND_K:                                # shorter than k: nothing happens
        assert not steps[7][1].any() and not steps[7][2].any()
    table = kmer.count_kmers(seq, meta, k=PM.HAND_K)
    try:
        for P in (1, 2, 3, 8):
            _all_forms(table, seq, meta, PM.HAND_T, P, steps[P - 1])
    finally:
        table.close()


def test_one_row_and_no_rows():
    import torch
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta, cases = PM.hand_rows()
    solid, _ = PM.solid_set(seq, meta, PM.HAND_K, PM.HAND_T)
    table = kmer.count_kmers(seq, meta, k=PM.HAND_K)
    try:
        for name in ('two_pass', 'three_pass_end'):
            row = cases[name][0]
            one, one_meta = seq[row:row + 1], meta[row:row + 1]
            steps = PM.trace(one, one_meta, PM.HAND_K, PM.HAND_T, 8, solid_keys=solid)
            assert steps[0][1][0] < steps[1][1][0]
            for P in (1, 2, 3, 8):
                _all_forms(table, one, one_meta, PM.HAND_T, P, steps[P - 1])
        # n = 0: nothing is launched, nothing is written
        lib = N.load()
        junk = torch.full((1, 48), 0xAA, dtype=torch.uint8, device='cuda')
        h, th = table.ctx.handle, table.handle
        assert lib.kbbq_kmer_correct_passes_dev(h, th, None, None, 0, 48, 3, None, None, 0, 2) == N.KBBQ_OK
        assert lib.kbbq_kmer_correct_passes_dev(h, th, N.ptr(junk), N.ptr(junk), 0, 48, 3, N.ptr(junk), N.ptr(junk), 0, 2) == N.KBBQ_OK
        assert lib.kbbq_kmer_flag_passes_dev(h, th, N.ptr(junk), N.ptr(junk), 0, 48, 3, N.ptr(junk), N.ptr(junk), N.ptr(junk),
                                             N.KMER_FLAG_UNRESOLVED, 2) == N.KBBQ_OK
        assert lib.kbbq_kmer_correct_rows_passes_dev(h, th, N.ptr(junk), N.ptr(junk), 0, 48, 0, 3, N.ptr(junk), N.ptr(junk), 0, 2) == N.KBBQ_OK
        assert lib.kbbq_kmer_correct_passes(h, th, None, None, 0, 48, 3, None, None, 0, 2) == N.KBBQ_OK
        table.ctx.status()
        assert int((junk != 0xAA).sum()) == 0
        empty = np.zeros((0, 48), dtype=np.uint8)
        out, ch = kmer.correct_with(table, empty, np.zeros(0, dtype=np.uint32), 3, passes=2)
        assert out.shape == (0, 48) and ch.shape == (0,)
        fl, ch, un = kmer.flag_errors(table, junk[:0], torch.zeros(0, dtype=torch.int32, device='cuda'), 3, unresolved=True, passes=2)
        assert tuple(fl.shape) == (0, 48) and tuple(ch.shape) == (0,) and tuple(un.shape) == (0,)
        # passes outside 1..8: refused before anything is launched, and the context stays usable
        for P in (0, 9):
            assert lib.kbbq_kmer_correct_passes_dev(h, th, N.ptr(junk), N.ptr(junk), 1, 48, 3, N.ptr(junk), N.ptr(junk), 0, P) == N.KBBQ_E_ARG
            assert 'passes must be in 1..8' in N.last_error()
        assert int((junk != 0xAA).sum()) == 0
        table.ctx.status()
    finally:
        table.close()


# ---------------------------------------------------------------- 2. the mixed-length set
def _mixed():
    if 'mixed' not in _memo:
        seq, meta = M.synth(7, genome_len=20000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
        seq.setflags(write=False); meta.setflags(write=False)
        _memo['mixed'] = (seq, meta)
    return _memo['mixed']


def _mixed_model(k):
    """(the model's steps after 1..4 passes, t) of the mixed set at k, computed once and left unchanged."""
    if ('mixed', k) not in _memo:
        seq, meta = _mixed()
        solid, t = PM.solid_set(seq, meta, k)
        _memo[('mixed', k)] = (_frozen(PM.trace(seq, meta, k, t, 4, solid_keys=solid)), t)
    return _memo[('mixed', k)]


@pytest.mark.parametrize('k', (15, 21, 31, 32))
def test_mixed_lengths_equal_the_model(k):
    from kbbq import kmer
    seq, meta = _mixed()
    assert seq.shape == (3571, 304) and 256 // (304 // 16) == 13 and 3571 % 13 != 0       # 13 rows a workgroup, the last one partial
    steps, t = _mixed_model(k)
    sums = [int(s[1].sum()) for s in steps]
    assert sums[0] + 50 <= sums[1] < sums[3]                                                # the set needs its later passes
    assert int((steps[0][2] == 2).sum()) > int((steps[1][2] == 2).sum()) > int((steps[3][2] == 2).sum()) >= 50
    assert int(steps[3][3].max()) == 4 and int(steps[3][3].min()) == 1                      # rows that end early, rows that do not
    table = kmer.count_kmers(seq, meta, k=k)
    try:
        assert kmer.solid_threshold(kmer.kmer_histogram(table)) == t
        for P in (2, 4):
            _all_forms(table, seq, meta, t, P, steps[P - 1])
    finally:
        table.close()


# ---------------------------------------------------------------- 3. one row of more than 256 chunks
def test_one_row_of_more_than_256_chunks():
    """4,100 bases, pitch 4,112: 257 chunks, one row a workgroup, every thread loops over chunks and thread 0 takes chunks 0 and
    256.  Errors by the two-pass recipe at the row's start, across the 256-chunk stride at its end, and three within k bases
    mid-row whose middle one has no window of its own before its neighbours are corrected."""
    from kbbq import kmer
    rng = np.random.default_rng(9)
    g = bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, 4100)])
    L = len(g)
    bad = PM._sub(g, 2, 8, 1594, 1601, 1608, 2500, L - 9, L - 3)
    seq, meta = M.plane([g] * 4 + [bad, PM._sub(g[200:350], 70, 80, 90)])
    assert seq.shape[1] == 4112 and seq.shape[1] // 16 > 256
    steps = PM.trace(seq, meta, 31, 3, 4)
    p1, p2 = steps[0][0][4], steps[1][0][4]
    truth = seq[0]
    assert p1[8] == truth[8] and p1[2] != truth[2] and p2[2] == truth[2]
    assert p1[L - 9] == truth[L - 9] and p1[L - 3] != truth[L - 3] and p2[L - 3] == truth[L - 3] and L - 3 >= 4096 > L - 9
    assert p1[1601] != truth[1601] and p2[1601] == truth[1601] and p1[2500] == truth[2500]
    assert np.array_equal(p2, truth) and steps[1][1][4] == 8
    assert steps[0][2][4, 4097] == 2 and steps[1][2][4, 4097] == 1
    table = kmer.count_kmers(seq, meta, k=31)
    try:
        for P in (2, 4):
            _all_forms(table, seq, meta, 3, P, steps[P - 1])
    finally:
        table.close()


def test_one_row_beyond_64_kb_of_lds():
    """40,000 bases: 2,500 chunks, 80 KB of LDS for the row's state -- more than a kernel may take without asking for it."""
    from kbbq import kmer
    rng = np.random.default_rng(10)
    g = bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, 40000)])
    L = len(g)
    seq, meta = M.plane([g] * 4 + [PM._sub(g, 2, 8, 20000, 20010, 20020, L - 9, L - 3)])
    assert (8 * (seq.shape[1] // 16) + 3) * 4 > 64 * 1024
    steps = PM.trace(seq, meta, 31, 3, 3)
    assert [int(s[1][4]) for s in steps] == [4, 7, 7] and np.array_equal(steps[1][0][4], seq[0])
    assert not np.array_equal(steps[1][2], steps[2][2])
    table = kmer.count_kmers(seq, meta, k=31)
    try:
        for P in (2, 3):
            _all_forms(table, seq, meta, 3, P, steps[P - 1])
    finally:
        table.close()


# ---------------------------------------------------------------- 4. without the model, and passes = 1
def test_p_passes_are_the_one_pass_kernel_applied_p_times():
    from kbbq import kmer
    seq, meta = _mixed()
    dseq, dmeta = _device(seq), _device(meta)
    table = kmer.count_kmers(dseq, dmeta, k=21)
    try:
        t = kmer.solid_threshold(kmer.kmer_histogram(table))
        x, planes = dseq, []
        for _ in range(3):
            x, _ = kmer.correct_with(table, x, dmeta, t, passes=1)       # the same table: nothing is recounted
            planes.append(_host(x))
        assert not np.array_equal(planes[0], planes[1]) and not np.array_equal(planes[1], planes[2])
        for P in (2, 3):
            out, changed = kmer.correct_with(table, dseq, dmeta, t, passes=P)
            assert np.array_equal(_host(out), planes[P - 1])
            assert np.array_equal(_host(changed).astype(np.int64), (planes[P - 1] != seq).sum(axis=1))
    finally:
        table.close()


def test_passes_1_is_the_existing_call_byte_for_byte():
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta = _mixed()
    dseq, dmeta = _device(seq), _device(meta)
    n, pitch = seq.shape
    lib = N.load()
    table = kmer.count_kmers(dseq, dmeta, k=31)

    def fresh():
        return (torch.full((n, pitch), 0xAA, dtype=torch.uint8, device='cuda'), torch.full((n,), -1, dtype=torch.int32, device='cuda'),
                torch.full((n,), -1, dtype=torch.int32, device='cuda'))
    try:
        t = kmer.solid_threshold(kmer.kmer_histogram(table))
        h, th = table.ctx.handle, table.handle
        for opts in (0, N.KMER_FIX_N):
            a, b = fresh(), fresh()
            N.check(lib.kbbq_kmer_correct_ex_dev(h, th, N.ptr(dseq), N.ptr(dmeta), n, pitch, t, N.ptr(a[0]), N.ptr(a[1]), opts))
            N.check(lib.kbbq_kmer_correct_passes_dev(h, th, N.ptr(dseq), N.ptr(dmeta), n, pitch, t, N.ptr(b[0]), N.ptr(b[1]), opts, 1))
            table.ctx.status()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int((a[0] != dseq).sum()) > 0
            ha, hb = np.full((n, pitch), 0xAA, dtype=np.uint8), np.full((n, pitch), 0xAA, dtype=np.uint8)
            ca, cb = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            N.check(lib.kbbq_kmer_correct_ex(h, th, N.ptr(seq), N.ptr(meta), n, pitch, t, N.ptr(ha), N.ptr(ca), opts))
            N.check(lib.kbbq_kmer_correct_passes(h, th, N.ptr(seq), N.ptr(meta), n, pitch, t, N.ptr(hb), N.ptr(cb), opts, 1))
            assert np.array_equal(ha, hb) and np.array_equal(ca, cb) and np.array_equal(ha, _host(a[0]))
            a, b = fresh(), fresh()
            N.check(lib.kbbq_kmer_correct_rows_ex_dev(h, th, N.ptr(dseq), N.ptr(dmeta), n, pitch, 0, t, N.ptr(a[0]), N.ptr(a[1]), opts))
            N.check(lib.kbbq_kmer_correct_rows_passes_dev(h, th, N.ptr(dseq), N.ptr(dmeta), n, pitch, 0, t, N.ptr(b[0]), N.ptr(b[1]), opts, 1))
            table.ctx.status()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for opts in (0, N.KMER_FLAG_UNRESOLVED):
            a, b = fresh(), fresh()
            N.check(lib.kbbq_kmer_flag_ex_dev(h, th, N.ptr(dseq), N.ptr(dmeta), n, pitch, t, N.ptr(a[0]), N.ptr(a[1]), N.ptr(a[2]), opts))
            N.check(lib.kbbq_kmer_flag_passes_dev(h, th, N.ptr(dseq), N.ptr(dmeta), n, pitch, t, N.ptr(b[0]), N.ptr(b[1]), N.ptr(b[2]), opts, 1))
            table.ctx.status()
            assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[0].sum()) > 0
        # 4-bit planes through the resident-rows call
        batch = dev.lay_out(_batch(seq, meta), 1)
        assert batch.layout_key() == 'reads_nib'
        c1 = _host(kmer.correct_batch(table, batch, t))
        first = _host(batch.cseq).copy()
        batch.cseq.fill_(0xAA)
        flags = dev._row_flags(batch)
        chg = torch.full((batch.n,), -1, dtype=torch.int32, device='cuda')
        N.check(lib.kbbq_kmer_correct_rows_passes_dev(h, th, N.ptr(batch.seq), N.ptr(batch.meta), batch.n, batch.pitch, flags, t,
                                                      N.ptr(batch.cseq), N.ptr(chg), 0, 1))
        table.ctx.status()
        assert np.array_equal(_host(batch.cseq), first) and np.array_equal(_host(chg), c1)
    finally:
        table.close()


# ---------------------------------------------------------------- 5. the N rule
def test_fix_n_two_passes_equal_the_model():
    import kmer_fixn_model as F
    from kbbq import kmer
    k = 21
    seq, meta, cases = F.with_ns(3, k)
    solid, t = PM.solid_set(seq, meta, k)
    steps = PM.trace(seq, meta, k, t, 2, fix_n=True, solid_keys=solid)
    inside = (seq == PM.NCH) & (np.arange(seq.shape[1])[None, :] < meta.astype(np.int64)[:, None])
    first, second = inside & (steps[0][0] != PM.NCH), inside & (steps[1][0] != PM.NCH)
    assert int(first.sum()) >= 1000 and int((second & ~first).sum()) >= 20                 # Ns that only the second pass fixes
    assert (inside & (steps[1][0] == PM.NCH)).any()                                         # ... and Ns that stay
    assert np.array_equal(steps[0][0], F.correct(seq, meta, k, t)[0])                       # pass 1 is the N rule's own model
    plain = PM.passes(seq, meta, k, t, 2, solid_keys=solid)
    assert not (inside & (plain[0] != PM.NCH)).any()                                        # without fix_n no N is touched
    table = kmer.count_kmers(seq, meta, k=k)
    try:
        assert kmer.solid_threshold(kmer.kmer_histogram(table)) == t
        _all_forms(table, seq, meta, t, 2, steps[1], fix_n=True)
        _all_forms(table, seq, meta, t, 2, plain)
    finally:
        table.close()


# ---------------------------------------------------------------- 6. resident rows
def _qual(seq, lens):
    q = np.full(seq.shape, 33 + 30, dtype=np.uint8)
    q[np.arange(seq.shape[1])[None, :] >= np.asarray(lens, dtype=np.int64)[:, None]] = 0
    return q


def _batch(seq, meta):
    from kbbq import _device as dev
    meta = np.asarray(meta, dtype=np.uint32)
    return dev.ReadBatch.from_host(np.array(seq), _qual(seq, meta & 0xFFFF), meta)       # a writable copy of the shared input


def test_four_bit_planes_two_passes():
    from kbbq import _device as dev
    from kbbq import kmer
    seq, meta = _mixed()
    steps, t = _mixed_model(31)
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'reads_nib' and laid.cseq is None and laid.n == seq.shape[0]
    lens = _host(laid.meta[:laid.n]).view(np.uint32) & 0xFFFF
    assert np.array_equal(lens, meta & 0xFFFF)           # one read group: the rows are the reads, in their order
    inside = np.arange(seq.shape[1])[None, :] < lens.astype(np.int64)[:, None]
    table = kmer.count_batch(laid, k=31)
    try:
        for P, fix_n in ((2, False), (4, False)):
            changed = kmer.correct_batch(table, laid, t, passes=P)
            got = _host(laid.chars('cseq')[:laid.n])[:, :seq.shape[1]]
            want = steps[P - 1]
            assert np.array_equal(got[inside], want[0][inside])
            assert np.array_equal(_host(changed).astype(np.int64), want[1])
    finally:
        table.close()


def test_four_bit_reads_fix_n_two_passes():
    """One read to a row of 4-bit codes with the N rule at two passes, the one selection of (reader, N rule, one pass / several)
    no other test reaches.  The hand-built rows with three Ns: one alone mid-read (pass 1 fixes it), one at a read's first base
    beside errors, and one at base 2 of the read whose base 8 is substituted -- every window over that N holds base 8, so pass 1
    corrects base 8 and leaves the N, and pass 2 fixes it."""
    from kbbq import _device as dev
    from kbbq import kmer
    seq, meta, cases = PM.hand_rows(pitch=48)
    seq = seq.copy()
    late, alone = cases['two_pass'][0], cases['truth'][0]
    seq[late, 2] = seq[alone, 20] = seq[cases['three_pass_end'][0], 0] = PM.NCH
    steps = PM.trace(seq, meta, PM.HAND_K, PM.HAND_T, 2, fix_n=True)
    truth = PM.hand_rows(pitch=48)[0][alone]
    assert steps[0][0][alone, 20] == truth[20] and steps[0][0][late, 8] == truth[8]
    assert steps[0][0][late, 2] == PM.NCH and steps[1][0][late, 2] == truth[2]
    assert int(steps[0][1].sum()) < int(steps[1][1].sum())
    laid = dev.lay_out(_batch(seq, meta), 1, pairs=False)
    assert laid.layout_key() == 'reads_nib' and laid.n == seq.shape[0]
    lens = _host(laid.meta[:laid.n]).view(np.uint32) & 0xFFFF
    assert np.array_equal(lens, meta & 0xFFFF)           # one read group: the rows are the reads, in their order
    inside = np.arange(seq.shape[1])[None, :] < lens.astype(np.int64)[:, None]
    was = _host(laid.chars('seq')[:laid.n])[:, :seq.shape[1]]
    table = kmer.count_batch(laid, k=PM.HAND_K)
    try:
        changed = kmer.correct_batch(table, laid, PM.HAND_T, fix_n=True, passes=2)
        got = _host(laid.chars('cseq')[:laid.n])[:, :seq.shape[1]]
        assert np.array_equal(got[inside], steps[1][0][inside]) and np.array_equal(got[~inside], was[~inside])
        assert np.array_equal(_host(changed).astype(np.int64), steps[1][1])
    finally:
        table.close()


def test_pair_rows_two_passes():
    """Two reads of 50 bases to a row of 4-bit codes (pitch 112) and of characters: each half of a row is the model's plane of
    the unpacked read, and a row's count is the sum of its two reads'."""
    from kbbq import _device as dev
    from kbbq import kmer
    S = 50
    seq, meta = M.synth(70, genome_len=5000, depth=30, err=0.02, len_lo=S, len_hi=S, n_rate=0.002)[:2]
    n = seq.shape[0] & ~1
    seq, meta = seq[:n], meta[:n].copy()
    solid, t = PM.solid_set(seq, meta, 21)
    steps = PM.trace(seq, meta, 21, t, 2, solid_keys=solid)
    fixn = PM.passes(seq, meta, 21, t, 2, fix_n=True, solid_keys=solid)
    assert int(steps[0][1].sum()) + 20 <= int(steps[1][1].sum()) < int(fixn[1].sum())
    paired = meta.copy()
    paired[1::2] |= SECOND
    for packed, key in ((True, 'pairs_nib'), (False, 'pairs')):
        laid = dev.lay_out(_batch(seq, paired), 1, packed=packed)
        assert laid.layout_key() == key and laid.pitch == 112 and laid.n == n // 2
        table = kmer.count_batch(laid, k=21)
        try:
            for want, fix_n in ((steps[1], False), (fixn, True)):
                changed = kmer.correct_batch(table, laid, t, fix_n=fix_n, passes=2)
                got = _host(laid.chars('cseq')[:laid.n])
                assert np.array_equal(got[:, :S], want[0][0::2, :S]) and np.array_equal(got[:, S + 1:2 * S + 1], want[0][1::2, :S])
                assert np.array_equal(_host(changed).astype(np.int64), want[1][0::2] + want[1][1::2])
        finally:
            table.close()


# ---------------------------------------------------------------- 7. the commands
def _kbbq(*argv, timeout=600):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + [str(a) for a in argv], capture_output=True, timeout=timeout, env=ENV)


def _fastq_text(names, seq, qual, meta):
    lens = np.asarray(meta, dtype=np.int64) & 0xFFFF
    return ''.join('@%s\n%s\n+\n%s\n' % (names[i], seq[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                   for i in range(seq.shape[0]))


@pytest.fixture(scope='module')
def fastq(tmp_path_factory):
    """reads.fq of the mixed set (shortest reads first: `recalibrate` takes non-decreasing lengths), three read groups in the
    names, what the model says `correct --passes 2` writes, and what the command wrote."""
    seq, meta = _mixed()
    steps, t = _mixed_model(31)
    d = tmp_path_factory.mktemp('passes')
    order = np.argsort(meta, kind='stable')
    rng = np.random.default_rng(8)
    names = ['r%d_RG:Z:g%d' % (i, g) for i, g in enumerate(rng.integers(0, 3, seq.shape[0]))]
    qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    fq = d / 'reads.fq'
    fq.write_text(_fastq_text(names, seq[order], qual, meta[order]))
    want = {P: _fastq_text(names, steps[P - 1][0][order], qual, meta[order]).encode() for P in (1, 2)}
    assert want[1] != want[2]
    out = d / 'one.fq'
    r = _kbbq('correct', '-f', fq, '--passes', '2', '-o', out)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return dict(dir=d, fq=str(fq), want=want, t=t, n=seq.shape[0], changed={P: int(steps[P - 1][1].sum()) for P in (1, 2)},
                one=out, stderr=r.stderr.decode())


def test_correct_passes_writes_the_models_fastq(fastq):
    assert fastq['one'].read_bytes() == fastq['want'][2]
    lines = re.findall(r'^kbbq correct: k=.*$', fastq['stderr'], flags=re.M)
    assert lines == ['kbbq correct: k=31 min_count=%d reads=%d changed_bases=%d passes=2' % (fastq['t'], fastq['n'], fastq['changed'][2])]
    # --passes 1 and no option: the bytes and the line of before
    for more in ((), ('--passes', '1')):
        r = _kbbq('correct', '-f', fastq['fq'], *more)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert r.stdout == fastq['want'][1]
        assert re.findall(r'^kbbq correct: k=.*$', r.stderr.decode(), flags=re.M) == [
            'kbbq correct: k=31 min_count=%d reads=%d changed_bases=%d' % (fastq['t'], fastq['n'], fastq['changed'][1])]
    # with the prefilter: the same bytes, passes=2 before the prefilter's figures
    r = _kbbq('correct', '-f', fastq['fq'], '--passes', '2', '--prefilter')
    assert r.returncode == 0 and r.stdout == fastq['want'][2]
    assert re.search(r'changed_bases=%d passes=2 prefilter=1 admitted=\d+ slots=\d+$' % fastq['changed'][2], r.stderr.decode(), re.M)


def _port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _launch(world, script, argv, env=None, timeout=400):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'), **(env or {}))
    env.setdefault('KBBQ_DIST_BACKEND', 'gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr',
           '127.0.0.1', '--master-port', str(_port()), os.path.join(ROOT, 'tests', script)] + list(argv)
    return subprocess.run(cmd, env=env, capture_output=True, timeout=timeout)


def test_three_ranks_write_the_one_process_bytes(fastq, tmp_path):
    out = str(tmp_path / 'out.fq')
    r = _launch(RANKS, 'dist_cli_worker.py', ['correct', '-f', fastq['fq'], '--passes', '2', '-o', out])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    parts = sorted(glob.glob(out + '.rank*'))
    assert len(parts) == RANKS
    assert b''.join(open(p, 'rb').read() for p in parts) == fastq['one'].read_bytes() == fastq['want'][2]
    lines = re.findall(r'^kbbq correct: k=.*$', r.stderr.decode(), flags=re.M)
    assert lines == re.findall(r'^kbbq correct: k=.*$', fastq['stderr'], flags=re.M) and len(lines) == 1
    assert lines[0].endswith(' passes=2')


def test_recalibrate_c_passes_equals_the_two_commands(fastq):
    two = _kbbq('recalibrate', '-f', fastq['fq'], fastq['one'], '--infer-rg')
    assert two.returncode == 0, two.stderr.decode()[-3000:]
    r = _kbbq('recalibrate', '-c', fastq['fq'], '--passes', '2', '--infer-rg')
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == two.stdout and len(two.stdout) > 0
    lines = [x for x in r.stderr.decode().splitlines() if x.startswith('kbbq recalibrate:')]
    assert lines == ['kbbq recalibrate: k=31 min_count=%d reads=%d changed_bases=%d passes=2' % (fastq['t'], fastq['n'], fastq['changed'][2])]
    one = _kbbq('recalibrate', '-c', fastq['fq'], '--infer-rg')
    assert one.returncode == 0 and one.stdout != r.stdout                # the second pass changes the model


@pytest.fixture(scope='module')
def alignments(tmp_path_factory):
    """The alignments of tests/test_gpu_kmer_unresolved.py (600 records of 60 bases, three read groups) and the model's final
    flag plane after two passes at k = 15."""
    import kmer_bqsr_model as B
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('passes_aln')
    paths = OQ.synth_bqsr_set(str(d), **B.FIXTURE)
    reads, rgs, pus = B.load(paths['sam'])
    seq, meta = B.planes(reads)
    solid, t = PM.solid_set(seq, meta, 15)
    steps = PM.trace(seq, meta, 15, t, 2, solid_keys=solid)
    assert int((steps[0][2] == 2).sum()) >= int((steps[1][2] == 2).sum()) + 50 and int(steps[1][1].sum()) > int(steps[0][1].sum())
    return dict(paths=paths, reads=reads, rgs=rgs, pus=pus, t=t, flags=steps[1][2], first=steps[0][2])


@pytest.mark.parametrize('skip', (False, True))
def test_bqsr_kmers_passes(alignments, skip, tmp_path):
    import kmer_bqsr_model as B
    import kmer_unresolved_model as U
    from kbbq.gatk import bqsr
    fx = alignments
    flags, t = fx['flags'], fx['t']
    if skip:
        want, winfo = U.vectors(fx['reads'], fx['rgs'], 15, classified=(flags, t))
        before, _ = U.vectors(fx['reads'], fx['rgs'], 15, classified=(fx['first'], t))
    else:
        want, winfo = B.vectors(fx['reads'], fx['rgs'], 15, flagged=(flags == 1, t))
        before, _ = B.vectors(fx['reads'], fx['rgs'], 15, flagged=(fx['first'] == 1, t))
    assert any(not np.array_equal(a, b) for a, b in zip(want, before))  # the second pass changes this fixture's tally
    model = tmp_path / 'model.grp'
    bqsr.vectors_to_report(*want, fx['pus']).write(str(model))
    grp = tmp_path / 'got.grp'
    r = _kbbq('bqsr', '-b', fx['paths']['sam'], '--kmers', '-k', '15', '--passes', '2', '-g', grp, *(['--skip-unresolved'] if skip else []))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert grp.read_bytes() == model.read_bytes()
    line = 'kbbq bqsr: k=15 min_count=%d reads=600 flagged_bases=%d' % (t, int((flags == 1).sum()))
    if skip:
        line += ' skipped_bases=%d' % int((flags == 2).sum())
    assert [ln for ln in r.stderr.decode().split('\n') if ln.startswith('kbbq bqsr:')] == [line + ' passes=2']


def test_benchmark_kmers_passes(alignments):
    import kmer_benchmark_model as KB
    fx = alignments
    p = fx['paths']
    reads, ref, skips = KB.load(p)
    want, winfo = KB.joint(reads, ref, skips, 15, classified=(fx['flags'], fx['t']))
    first, _ = KB.joint(reads, ref, skips, 15, classified=(fx['first'], fx['t']))
    assert not np.array_equal(want, first)
    r = _kbbq('benchmark', '-b', p['sam'], '-r', p['fa'], '-v', p['vcf'], '--kmers', '-k', '15', '--passes', '2', '-l', 'lbl')
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode() == KB.render(want, 'lbl')
    assert [ln for ln in r.stderr.decode().split('\n') if ln.startswith('kbbq benchmark:')] == [KB.summary(winfo) + ' passes=2']
