"""kbbq correct --fix-n on the MI355X against the CPU model of the N rule (tests/kmer_fixn_model.py), byte for byte: planes on the
device and on the host, with the prefilter, the rule off against the existing calls, device batches in the four layouts of the
recalibrate path, a row of more than 256 chunks, the command line on one process and on three ranks, and `recalibrate -c
--fix-n` against the two commands it replaces."""
import ctypes
import glob
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import kmer_fixn_model as F
import kmer_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_SEQUENTIAL', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS'):
    ENV.pop(_var, None)
SECOND = np.uint32(1 << 31)
NCH = ord('N')

_memo = {}


def _reads(k):
    """The N-carrying read set for k and the model's answer, computed once and left unchanged."""
    if k not in _memo:
        seq, meta, cases = F.with_ns(7, k, genome_len=20000, depth=30)
        want, changed, t, kinds = F.correct(seq, meta, k)
        for a in (seq, meta, want, changed):
            a.setflags(write=False)
        n = F.kind_counts(kinds)
        assert n['fixed'] >= 100 and n['tie'] >= 1 and n['none'] >= 1 and n['second_break'] >= 1, n
        _memo[k] = (seq, meta, want, changed, t)
    return _memo[k]


def _device(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


@pytest.mark.parametrize('k', [15, 21, 31, 32])
def test_planes_on_the_device_and_on_the_host(k):
    from kbbq import kmer
    seq, meta, want, want_changed, t = _reads(k)
    table = kmer.count_kmers(seq, meta, k=k)
    try:
        assert kmer.solid_threshold(kmer.kmer_histogram(table)) == t
        out, changed = kmer.correct_with(table, seq, meta, t, fix_n=True)
        assert np.array_equal(out, want) and np.array_equal(changed.astype(np.int64), want_changed)
        dseq = _device(seq)
        dout, dchanged = kmer.correct_with(table, dseq, _device(meta), t, fix_n=True)
        assert np.array_equal(dout.cpu().numpy(), want) and np.array_equal(dchanged.cpu().numpy().astype(np.int64), want_changed)
        assert np.array_equal(dseq.cpu().numpy(), seq)             # the input plane is as it was
    finally:
        table.close()
    # ... and with the prefilter: the filter keeps keys of count 1 out, the rule asks for count >= t >= 2
    pout, info = kmer.correct_reads(seq, meta, k=k, prefilter=True, fix_n=True)
    assert info['min_count'] == t and info['fix_n'] is True and info['prefilter'] is True
    assert np.array_equal(pout, want) and np.array_equal(info['changed'].astype(np.int64), want_changed)


def test_the_rule_off_and_opts_zero_are_the_existing_calls():
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    k = 31
    seq, meta, want_on, _, t = _reads(k)
    plain, plain_changed, _ = F.substitutions(seq, meta, k, t)
    assert not np.array_equal(plain, want_on)
    table = kmer.count_kmers(seq, meta, k=k)
    lib, ctx = N.load(), table.ctx
    n, pitch = seq.shape
    try:
        off, off_changed = kmer.correct_with(table, seq, meta, t)
        assert np.array_equal(off, plain) and np.array_equal(off_changed.astype(np.int64), plain_changed)
        off2, _ = kmer.correct_with(table, seq, meta, t, fix_n=False)
        assert np.array_equal(off2, plain)
        # host buffers: the existing call and the _ex call with opts = 0
        outs = []
        for call, extra in ((lib.kbbq_kmer_correct, ()), (lib.kbbq_kmer_correct_ex, (0,))):
            out, ch = np.empty_like(seq), np.zeros(n, dtype=np.uint32)
            N.check(call(ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t, N.ptr(out), N.ptr(ch), *extra))
            outs.append((out, ch))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], plain)
        # device planes: _dev / _ex_dev, and the rows calls on the same character rows
        dseq, dmeta = _device(seq), _device(meta)
        douts = []
        for call, args in ((lib.kbbq_kmer_correct_dev, ()), (lib.kbbq_kmer_correct_ex_dev, (0,)),
                           (lib.kbbq_kmer_correct_rows_dev, None), (lib.kbbq_kmer_correct_rows_ex_dev, 0)):
            out, ch = torch.empty_like(dseq), torch.zeros(n, dtype=torch.int32, device='cuda')
            if isinstance(args, tuple):
                N.check(call(ctx.handle, table.handle, N.ptr(dseq), N.ptr(dmeta), n, pitch, t, N.ptr(out), N.ptr(ch), *args))
            else:
                N.check(call(ctx.handle, table.handle, N.ptr(dseq), N.ptr(dmeta), n, pitch, 0, t, N.ptr(out), N.ptr(ch),
                             *(() if args is None else (args,))))
            ctx.status()
            douts.append((out.cpu().numpy(), ch.cpu().numpy()))
        for out, ch in douts:
            assert np.array_equal(out, plain) and np.array_equal(ch.astype(np.int64), plain_changed)
        # an unknown bit is refused with a context and a table at hand too, and nothing is written
        out = torch.zeros_like(dseq)
        rc = lib.kbbq_kmer_correct_ex_dev(ctx.handle, table.handle, N.ptr(dseq), N.ptr(dmeta), n, pitch, t, N.ptr(out), None, 2)
        assert rc == N.KBBQ_E_ARG and 'opts' in N.last_error()
        torch.cuda.synchronize()
        assert not out.any()
        assert dev.context() is not None
    finally:
        table.close()


# ---- device batches in the recalibrate path's layouts -------------------------------------------------------------------------

def _qual(seq, lens):
    q = np.full(seq.shape, 33 + 30, dtype=np.uint8)
    q[np.arange(seq.shape[1])[None, :] >= np.asarray(lens, dtype=np.int64)[:, None]] = 0
    return q


def _batch(seq, meta):
    from kbbq import _device as dev
    meta = np.asarray(meta, dtype=np.uint32)
    return dev.ReadBatch.from_host(np.ascontiguousarray(seq), _qual(seq, meta & 0xFFFF), meta)


S_FIXED = 100


@pytest.fixture(scope='module')
def fixed():
    """Reads of one length with Ns: among them an N as the last base of a row's first read (an even read), as the first base of
    its second read (an odd read), both in one row, and at random.  The model's answer, one read a row, at k = 21."""
    k, S = 21, S_FIXED
    seq, meta, truth, _ = M.synth(41, genome_len=5000, depth=30, err=0.01, len_lo=S, len_hi=S)
    n = seq.shape[0] & ~1
    seq, meta, truth = seq[:n].copy(), meta[:n].copy(), truth[:n]
    rng = np.random.default_rng(42)
    seq[:, :S][rng.random((n, S)) < 0.003] = NCH
    seq[10], seq[13], seq[20], seq[21] = truth[10], truth[13], truth[20], truth[21]
    seq[10, S - 1] = NCH                                       # last base of row 5's first read
    seq[13, 0] = NCH                                           # first base of row 6's second read
    seq[20, S - 1] = seq[21, 0] = NCH                          # both sides of row 10's separator
    want, changed, t, kinds = F.correct(seq, meta, k)
    for at in ((10, S - 1), (13, 0), (20, S - 1), (21, 0)):
        assert kinds[at] == 'fixed'
    n_kinds = F.kind_counts(kinds)
    assert n_kinds['fixed'] >= 50 and n_kinds['none'] >= 1
    return k, seq, meta, want, changed, t


def _as_pair_rows(plane, S, pitch):
    """One-read-per-row characters -> the characters of rows of two reads ([first][N][second][N ...]); an odd count: the last
    row's second half is padding."""
    n = plane.shape[0]
    rows = np.full(((n + 1) // 2, pitch), NCH, dtype=np.uint8)
    rows[:, :S] = plane[0::2, :S]
    rows[:n // 2, S + 1:2 * S + 1] = plane[1::2, :S]
    return rows


@pytest.mark.parametrize('layout', ['reads', 'reads_nib', 'pairs', 'pairs_nib', 'twins_odd'])
def test_batches_in_every_layout(fixed, layout):
    from kbbq import _device as dev
    from kbbq import kmer
    k, seq, meta, want, want_changed, t = fixed
    S = S_FIXED
    if layout == 'twins_odd':
        seq, meta, want, want_changed = seq[:-1], meta[:-1], want[:-1], want_changed[:-1]
        laid = dev.lay_out(_batch(seq, meta), 1)
        assert laid.layout_key() == 'pairs_nib' and laid.twins and laid.n == (seq.shape[0] + 1) // 2 and seq.shape[0] % 2 == 1
    elif layout == 'reads':
        laid = _batch(seq, meta)
    elif layout == 'reads_nib':
        laid = dev.lay_out(_batch(seq, meta), 1, pairs=False)
    else:
        paired = meta.copy()
        paired[1::2] |= SECOND
        laid = dev.lay_out(_batch(seq, paired), 1, packed=layout == 'pairs_nib')
        assert not laid.twins
    assert laid.layout_key() == ('pairs_nib' if layout == 'twins_odd' else layout) and laid.perm is None
    if isinstance(laid, dev.PairBatch):
        expect = _as_pair_rows(want, S, laid.pitch)
        was = _as_pair_rows(seq, S, laid.pitch)
        pairs = np.concatenate([want_changed, [0]])[:2 * laid.n].reshape(-1, 2).sum(axis=1)
    else:
        expect, was, pairs = want, seq, want_changed
    assert np.array_equal(laid.chars('seq')[:laid.n].cpu().numpy(), was)
    table = kmer.count_batch(laid, k=k)
    try:
        changed = kmer.correct_batch(table, laid, t, fix_n=True)
        got = laid.chars('cseq')[:laid.n].cpu().numpy()
        assert np.array_equal(got, expect)
        assert np.array_equal(changed.cpu().numpy().astype(np.int64), pairs)
        assert np.array_equal(laid.chars('seq')[:laid.n].cpu().numpy(), was)
        # ... and the rule off in the same layout: the substitutions alone
        plain = F.substitutions(seq, meta, k, t)[0]
        kmer.correct_batch(table, laid, t)
        off = laid.chars('cseq')[:laid.n].cpu().numpy()
        assert np.array_equal(off, _as_pair_rows(plain, S, laid.pitch) if isinstance(laid, dev.PairBatch) else plain)
    finally:
        table.close()


def test_a_character_row_of_more_than_256_chunks():
    from kbbq import kmer
    rng = np.random.default_rng(9)
    genome = rng.integers(0, 4, 4112)
    reads = []
    for L in (4112, 4112, 4112, 4111, 4100, 4097, 4112):
        x = genome[:L].copy()
        at = rng.choice(L, 4, replace=False)
        x[at] = (x[at] + rng.integers(1, 4, 4)) % 4
        y = np.frombuffer(M.LETTERS, dtype=np.uint8)[x].copy()
        y[rng.choice(L, 12, replace=False)] = NCH
        reads.append(bytes(y))
    seq, meta = M.plane(reads)
    seq[0, 0] = seq[1, 4095] = seq[1, 4096] = seq[2, 4111] = seq[3, 4110] = NCH   # the row's ends and the 256th chunk's edge
    assert seq.shape[1] == 4112 and seq.shape[1] // 16 == 257
    want, want_changed, t, kinds = F.correct(seq, meta, 31, 3)
    n = F.kind_counts(kinds)
    assert n['fixed'] >= 40 and kinds[(0, 0)] == kinds[(1, 4095)] == kinds[(3, 4110)] == 'fixed' and (2, 4111) in kinds
    table = kmer.count_kmers(seq, meta, k=31)
    try:
        out, changed = kmer.correct_with(table, _device(seq), _device(meta), 3, fix_n=True)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(changed.cpu().numpy().astype(np.int64), want_changed)
    finally:
        table.close()


# ---- the command line --------------------------------------------------------------------------------------------------------

def _kbbq(*argv, timeout=600):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + [str(a) for a in argv], capture_output=True, timeout=timeout, env=ENV)


def _fastq_text(names, seq, qual, meta):
    lens = np.asarray(meta, dtype=np.int64) & 0xFFFF
    return ''.join('@%s\n%s\n+\n%s\n' % (names[i], seq[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                   for i in range(seq.shape[0]))


@pytest.fixture(scope='module')
def fastq(tmp_path_factory):
    """reads.fq of the k = 31 set (shortest reads first: `recalibrate` takes non-decreasing lengths), three read groups in the
    names, and what the model says `correct --fix-n` writes."""
    seq, meta, want, want_changed, t = _reads(31)
    d = tmp_path_factory.mktemp('fixn')
    order = np.argsort(meta, kind='stable')
    seq, meta, want, want_changed = seq[order], meta[order], want[order], want_changed[order]
    rng = np.random.default_rng(8)
    names = ['r%d_RG:Z:g%d' % (i, g) for i, g in enumerate(rng.integers(0, 3, seq.shape[0]))]
    qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    fq = d / 'reads.fq'
    fq.write_text(_fastq_text(names, seq, qual, meta))
    return dict(dir=d, fq=str(fq), want=_fastq_text(names, want, qual, meta).encode(), changed=int(want_changed.sum()), t=t,
                n=seq.shape[0], meta=meta)


@pytest.fixture(scope='module')
def one_process(fastq):
    out = fastq['dir'] / 'one.fq'
    r = _kbbq('correct', '-f', fastq['fq'], '--fix-n', '-o', out)
    assert r.returncode == 0, r.stderr.decode()
    return out, r


def test_correct_fix_n_writes_the_models_fastq(fastq, one_process):
    out, r = one_process
    assert out.read_bytes() == fastq['want']
    lines = [x for x in r.stderr.decode().splitlines() if x.startswith('kbbq correct:')]
    assert lines == ['kbbq correct: k=31 min_count=%d reads=%d changed_bases=%d fix_n=1' % (fastq['t'], fastq['n'], fastq['changed'])]
    # without the flag: the line as it was, fewer changed bases, and every N as read
    plain = _kbbq('correct', '-f', fastq['fq'])
    assert plain.returncode == 0, plain.stderr.decode()
    m = re.search(r'^kbbq correct: k=31 min_count=%d reads=%d changed_bases=(\d+)$' % (fastq['t'], fastq['n']), plain.stderr.decode(), re.M)
    assert m and int(m.group(1)) < fastq['changed']
    assert plain.stdout.count(b'N') == open(fastq['fq'], 'rb').read().count(b'N') > out.read_bytes().count(b'N')
    # with the prefilter: the same bytes, fix_n=1 before the prefilter's figures
    pre = _kbbq('correct', '-f', fastq['fq'], '--fix-n', '--prefilter')
    assert pre.returncode == 0 and pre.stdout == fastq['want']
    assert re.search(r'changed_bases=%d fix_n=1 prefilter=1 admitted=\d+ slots=\d+$' % fastq['changed'], pre.stderr.decode(), re.M)


def test_the_command_does_not_import_torch(fastq, tmp_path):
    out = tmp_path / 'out.fq'
    code = ('import sys\nfrom kbbq import main\nmain.main(["correct", "-f", %r, "--fix-n", "-o", %r])\n'
            'assert "torch" not in sys.modules, "torch was imported"\nprint("no torch")\n' % (fastq['fq'], str(out)))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, timeout=600, env=ENV)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b'no torch\n' and out.read_bytes() == fastq['want']


def test_recalibrate_c_fix_n_equals_the_two_commands(fastq, one_process, tmp_path):
    from kbbq import fastx
    assert len(fastx.length_bands(fastq['meta'])) >= 4
    cor, _ = one_process
    two = _kbbq('recalibrate', '-f', fastq['fq'], cor, '--infer-rg')
    assert two.returncode == 0, two.stderr.decode()
    r = _kbbq('recalibrate', '-c', fastq['fq'], '--fix-n', '--infer-rg')
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == two.stdout and len(two.stdout) > 0
    lines = [x for x in r.stderr.decode().splitlines() if x.startswith('kbbq recalibrate:')]
    assert lines == ['kbbq recalibrate: k=31 min_count=%d reads=%d changed_bases=%d fix_n=1' % (fastq['t'], fastq['n'], fastq['changed'])]
    # the fixed Ns matter to the model: without the flag the qualities differ
    off = _kbbq('recalibrate', '-c', fastq['fq'], '--infer-rg')
    assert off.returncode == 0 and off.stdout != r.stdout and b'fix_n' not in off.stderr


# ---- ranks -------------------------------------------------------------------------------------------------------------------

RANKS = 3


def _port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def test_three_ranks_write_the_one_process_bytes(fastq, one_process, tmp_path):
    out = str(tmp_path / 'out.fq')
    env = dict(ENV, HSA_ENABLE_IPC_MODE_LEGACY='0', KBBQ_DIST_BACKEND='gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(RANKS), '--master-addr',
           '127.0.0.1', '--master-port', str(_port()), os.path.join(ROOT, 'tests', 'dist_cli_worker.py'),
           'correct', '-f', fastq['fq'], '--fix-n', '-o', out]
    r = subprocess.run(cmd, env=env, capture_output=True, timeout=400)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    parts = sorted(glob.glob(out + '.rank*'))
    assert len(parts) == RANKS
    assert b''.join(open(p, 'rb').read() for p in parts) == one_process[0].read_bytes() == fastq['want']
    lines = re.findall(r'^kbbq correct: k=.*$', r.stderr.decode(), flags=re.M)
    assert lines == re.findall(r'^kbbq correct: k=.*$', one_process[1].stderr.decode(), flags=re.M) and len(lines) == 1
    assert lines[0].endswith(' fix_n=1')
