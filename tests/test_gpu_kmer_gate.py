"""`--kmer-min-qual Q` on the MI355X: km_gate (kbbq_kmer_gate_rows_dev, kbbq.kmer gate_plane / gate_batch) against the CPU model
of the rule (tests/kmer_gate_model.py) -- the gated plane byte for byte and the counted windows -- on character rows and in
every layout of the recalibrate path, at the chunk edges, on rows of more than 256 chunks, on a raw-Phred plane, without a
window word and with two calls into one; its refusals; the gate in front of the count, the prefilter and the partition rounds
(entries, histogram, threshold, corrected plane on the two fixtures); and the commands, each in a child process, byte for byte
against the model and against the command without the option: `correct` (stdout and the stderr line) and `recalibrate -c` (which
is `correct --kmer-min-qual` followed by `recalibrate -f`) on fixture F1; `bqsr --kmers` (the report text), `recalibrate -b --kmers`
(which is that command followed by `applybqsr`) and `benchmark --kmers` on the aligned fixtures of tests/test_gpu_bqsr_mixed.py,
since F1's reads have no alignments; `correct` on two ranks.  Exact equality throughout."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmer_gate_model as G
import kmer_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_SEQUENTIAL', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_DEVICE_BUDGET', 'KBBQ_TALLY_FUSED'):
    ENV.pop(_var, None)
SECOND = np.uint32(1 << 31)


def _batch(seq, meta, qual=None):
    from kbbq import _device as dev
    meta = np.array(meta, dtype=np.uint32)
    return dev.ReadBatch.from_host(np.array(seq), np.array(G.quals(seq, meta) if qual is None else qual), meta)


def _rows(batch, name='seq'):
    """(characters [n, pitch], sidecar lengths) of a laid batch."""
    chars = batch.chars(name)[:batch.n].cpu().numpy()
    lens = batch.meta[:batch.n].cpu().numpy().view(np.uint32) & 0xFFFF
    return chars, lens


def _check(batch, k, Q):
    """gate_batch of `batch` against the model of its own rows and quality plane; counting the gated plane inserts exactly the
    counted windows, and they are the model's k-mers."""
    from kbbq import kmer
    chars, lens = _rows(batch)
    raw = batch.seq.cpu().numpy().copy()
    qual = batch.qual[:batch.n].cpu().numpy().copy()
    want = G.gate(chars, qual, Q + 33)
    valid = M.windows(want, lens, k)[2]
    inside = np.arange(chars.shape[1])[None, :] < lens.astype(np.int64)[:, None]
    low = int((inside & (qual < Q + 33)).sum())
    assert 0 < low < int(inside.sum())                               # some but not all bases are gated
    assert 0 < int(valid.sum()) < int(M.windows(chars, lens, k)[2].sum())
    plane, windows = kmer.gate_batch(batch, k, Q)
    assert plane.shape == batch.seq.shape and plane.data_ptr() != batch.seq.data_ptr()
    batch.gated = plane
    assert np.array_equal(batch.chars('gated')[:batch.n].cpu().numpy(), want)
    assert windows == int(valid.sum())
    assert np.array_equal(batch.seq.cpu().numpy(), raw) and np.array_equal(batch.qual[:batch.n].cpu().numpy(), qual)
    table = kmer.count_batch(batch, k=k, plane=plane)
    keys, counts = table.entries()
    table.close()
    wk, wc = M.count(want, lens, k)
    assert np.array_equal(keys, wk) and np.array_equal(counts.astype(np.int64), wc) and int(wc.sum()) == windows
    return want, windows


@pytest.fixture(scope='module')
def mixed():
    f = G.fixture('F2')
    return f['seq'], f['meta'], f['qual']


def _fixed(seed, S, paired=True):
    seq, meta = M.synth(seed, genome_len=5000, depth=30, err=0.01, len_lo=S, len_hi=S)[:2]
    n = seq.shape[0] & ~1
    seq, meta = seq[:n], meta[:n].copy()
    if paired:
        meta[1::2] |= SECOND
    return seq, meta


# ---------------------------------------------------------------- the kernel against the model
@pytest.mark.parametrize('k', [8, 15, 31, 32])
def test_character_rows(mixed, k):
    seq, meta, qual = mixed
    batch = _batch(seq, meta, qual)
    assert batch.layout_key() == 'reads' and batch.n % max(1, 256 // (batch.pitch // 16)) != 0     # the last workgroup is short
    want, windows = _check(batch, k, 20)
    if k == 31:
        f = G.fixture('F2')
        assert np.array_equal(want, f['gated']) and windows == f['windows'] == 74515


@pytest.mark.parametrize('k', [8, 15, 31, 32])
def test_reads_nib(mixed, k):
    from kbbq import _device as dev
    seq, meta, qual = mixed
    laid = dev.lay_out(_batch(seq, meta, qual), 1)
    assert laid.layout_key() == 'reads_nib'
    _check(laid, k, 20)


@pytest.mark.parametrize('packed', [False, True])
def test_pairs(packed):
    from kbbq import _device as dev
    seq, meta = _fixed(70, 50)
    laid = dev.lay_out(_batch(seq, meta), 1, packed=packed)
    assert laid.layout_key() == ('pairs_nib' if packed else 'pairs') and laid.pitch == 112 and not laid.twins
    assert set(_rows(laid)[1].tolist()) == {101}
    _check(laid, 21, 20)


def test_twins_with_an_odd_number_of_reads():
    from kbbq import _device as dev
    seq, meta = _fixed(31, 100, paired=False)
    seq, meta = seq[:-1], meta[:-1]
    assert seq.shape[0] % 2 == 1
    laid = dev.lay_out(_batch(seq, meta), 1)
    assert laid.layout_key() == 'pairs_nib' and laid.twins and laid.n == (seq.shape[0] + 1) // 2
    _check(laid, 31, 20)


def test_rows_grouped_by_read_group(mixed):
    from kbbq import _device as dev
    seq, meta, qual = mixed
    rng = np.random.default_rng(5)
    meta = meta | (rng.integers(0, 3, meta.size).astype(np.uint32) << np.uint32(16))
    laid = dev.lay_out(_batch(seq, meta, qual), 3)
    assert laid.layout_key() == 'reads_nib' and laid.seg is not None and laid.perm is not None
    _, windows = _check(laid, 21, 20)
    assert windows == G.counted_windows(seq, qual, meta, 21, 53)      # grouping only orders the rows


@pytest.mark.parametrize('nib', [False, True])
def test_chunk_edges(nib):
    from kbbq import _device as dev
    rng = np.random.default_rng(3)
    genome = rng.integers(0, 4, 600)
    reads = []
    for L in (0, 5, 14, 15, 16, 17, 30, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81):
        for _ in range(40 if L else 1):
            s = int(rng.integers(0, 600 - L + 1))
            reads.append(bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[genome[s:s + L]]))
    seq, meta = M.plane(reads)
    batch = _batch(seq, meta)
    if nib:
        batch = dev.lay_out(batch, 1)
    assert batch.layout_key() == ('reads_nib' if nib else 'reads') and 0 in _rows(batch)[1].tolist()
    for k in (8, 15, 32):
        _check(batch, k, 13)                                         # {2, 12} are gated: runs of ~65 countable bases


@pytest.mark.parametrize('nib', [False, True])
def test_rows_of_more_than_256_chunks(nib):
    from kbbq import _device as dev
    rng = np.random.default_rng(9)
    genome = rng.integers(0, 4, 4112)
    reads = [bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[genome[:L]]) for L in (4112, 4112, 4112, 4111, 4100, 4097, 4112)]
    seq, meta = M.plane(reads)
    batch = _batch(seq, meta)
    if nib:
        batch = dev.lay_out(batch, 1)
    assert batch.pitch // 16 == 257
    _check(batch, 31, 20)


def test_raw_phred_plane_without_a_window_word_and_two_calls_into_one(mixed):
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta, qual = mixed
    k, Q = 31, 20
    f = G.fixture('F2')
    raw = np.where(qual >= 33, qual - 33, 0).astype(np.uint8)
    assert np.array_equal(G.gate(seq, raw, Q), f['gated'])
    plane, windows = kmer.gate_plane(seq, raw, meta, k, Q, qual_offset=0)            # host arrays are uploaded
    assert np.array_equal(plane.cpu().numpy(), f['gated']) and windows == f['windows']
    # no window word: the plane alone
    d = [torch.from_numpy(np.array(a)).cuda() for a in (seq, qual, meta.view(np.int32))]
    out = torch.zeros_like(d[0])
    lib, ctx = N.load(), dev.context()
    N.check(lib.kbbq_kmer_gate_rows_dev(ctx.handle, N.ptr(d[0]), N.ptr(d[1]), N.ptr(d[2]), seq.shape[0], seq.shape[1], 0, k, Q + 33,
                                        N.ptr(out), None))
    ctx.status()
    assert np.array_equal(out.cpu().numpy(), f['gated'])
    # two calls add into one word; nrows == 0 does nothing
    h = seq.shape[0] // 2 + 1
    word = torch.zeros(1, dtype=torch.int64, device='cuda')
    first = kmer.gate_plane(d[0][:h], d[1][:h], d[2][:h], k, Q, windows=word)
    both = kmer.gate_plane(d[0][h:], d[1][h:], d[2][h:], k, Q, windows=word)
    assert 0 < first[1] < both[1] == f['windows']
    assert np.array_equal(np.concatenate([first[0].cpu().numpy(), both[0].cpu().numpy()]), f['gated'])
    N.check(lib.kbbq_kmer_gate_rows_dev(ctx.handle, None, None, None, 0, 16, 0, k, Q + 33, None, N.ptr(word)))
    ctx.status()
    assert int(word.cpu()[0]) == f['windows']
    assert np.array_equal(d[0].cpu().numpy(), seq) and np.array_equal(d[1].cpu().numpy(), qual)


def test_refusals(mixed):
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    seq, meta, qual = mixed
    laid = dev.lay_out(_batch(seq, meta, qual), 1)
    lib, ctx = N.load(), dev.context()
    out = torch.empty_like(laid.seq)
    word = torch.zeros(1, dtype=torch.int64, device='cuda')
    off = torch.empty(laid.seq.numel() + 64, dtype=torch.uint8, device='cuda')[4:]
    good = dict(seq=N.ptr(laid.seq), qual=N.ptr(laid.qual), meta=N.ptr(laid.meta), n=laid.n, pitch=laid.pitch, flags=N.ROWS_NIBBLES,
                k=31, qmin=53, out=N.ptr(out), windows=N.ptr(word))

    def call(**kw):
        a = dict(good, **kw)
        N.check(lib.kbbq_kmer_gate_rows_dev(ctx.handle, a['seq'], a['qual'], a['meta'], a['n'], a['pitch'], a['flags'], a['k'], a['qmin'],
                                            a['out'], a['windows']))
    for kw, said in ((dict(seq=None), 'NULL'), (dict(qual=None), 'NULL'), (dict(meta=None), 'NULL'), (dict(out=None), 'NULL'),
                     (dict(out=good['seq']), 'd_out is d_seq'), (dict(seq=N.ptr(off)), 'aligned'), (dict(out=N.ptr(off)), 'aligned'),
                     (dict(qual=N.ptr(off)), 'aligned'), (dict(flags=0, seq=N.ptr(off)), 'aligned'), (dict(k=7), 'k must be in 8..32'),
                     (dict(k=33), 'k must be in 8..32'), (dict(qmin=0), r'qual_byte_min must be in 1..255'),
                     (dict(qmin=256), r'qual_byte_min must be in 1..255'), (dict(flags=8), 'flags'), (dict(flags=N.ROWS_TWINS), 'TWINS'),
                     (dict(pitch=laid.pitch + 8), 'pitch'), (dict(n=-1), 'nreads')):
        with pytest.raises(ValueError, match='kbbq_kmer_gate_rows_dev.*(%s)' % said):
            call(**kw)
    ctx.status()
    assert int(word.cpu()[0]) == 0                                   # nothing was launched
    call()                                                           # the context goes on working
    ctx.status()
    assert int(word.cpu()[0]) == G.fixture('F2')['windows']
    with pytest.raises(ValueError, match='1..93'):
        kmer.gate_batch(laid, 31, 94)
    with pytest.raises(ValueError, match='no quality plane'):
        kmer.gate_plane(seq, None, meta, 31, 20)


# ---------------------------------------------------------------- the gate in front of the count
def _entries(table):
    keys, counts = table.entries()
    table.close()
    return keys, counts.astype(np.int64)


@pytest.mark.parametrize('name', ['F1', 'F2'])
def test_the_gated_table_is_the_models(name):
    from kbbq import kmer
    f = G.fixture(name)
    G.assert_not_vacuous(f)
    plane, windows = kmer.gate_plane(f['seq'], f['qual'], f['meta'], f['k'], f['Q'])
    assert windows == f['windows'] == int(f['counts'].sum())
    import torch
    d_meta = torch.from_numpy(f['meta'].view(np.int32).copy()).cuda()
    table = kmer.count_kmers(plane, d_meta, k=f['k'], slots=kmer.default_slots(windows, 1 << 30))
    hist = kmer.kmer_histogram(table)
    keys, counts = _entries(table)
    assert np.array_equal(keys, f['keys']) and np.array_equal(counts, f['counts'])
    assert np.array_equal(hist, f['hist']) and kmer.solid_threshold(hist) == f['t'] < f['plain_t']


@pytest.mark.parametrize('name', ['F1', 'F2'])
@pytest.mark.parametrize('how', ['plain', 'prefilter', 'partitions', 'both'])
def test_correct_reads(name, how):
    from kbbq import kmer
    f = G.fixture(name)
    G.assert_not_vacuous(f)
    kw = dict(prefilter=how in ('prefilter', 'both'), **(dict(partitions=4) if how in ('partitions', 'both') else {}))
    out, info = kmer.correct_reads(f['seq'], f['meta'], k=f['k'], qual_plane=f['qual'], kmer_min_qual=f['Q'], **kw)
    ungated, plain = kmer.correct_reads(f['seq'], f['meta'], k=f['k'], **kw)
    assert np.array_equal(out, f['out']) and np.array_equal(np.asarray(info['changed']).astype(np.int64), f['changed'])
    lo = 2 if kw['prefilter'] else 0
    assert np.array_equal(info['hist'][lo:], f['hist'][lo:]) and info['min_count'] == f['t']
    assert (info['kmer_min_qual'], info['counted_windows']) == (f['Q'], f['windows'])
    assert info['windows'] == kmer.kmer_total(f['meta'], f['k']) >= f['plain_windows'] > f['windows']    # by the sidecars, Ns included
    assert info.get('partitions', 1) == (4 if 'partitions' in kw else 1)
    # the run without the option is what it was, and the gate saves what it is there to save
    assert np.array_equal(ungated, f['plain_out']) and plain['min_count'] == f['plain_t'] and 'kmer_min_qual' not in plain
    assert int((out != ungated).sum()) == (28 if name == 'F1' else 1)
    if not kw['prefilter']:
        assert info['slots'] <= plain['slots'] and info['table_bytes'] <= plain['table_bytes']
    if how == 'plain':
        # sized from the counted windows, not from the sidecars: a load factor of at most 0.5 (F2's two sizes round to one table)
        assert info['slots'] == kmer._wanted_slots(f['windows']) and plain['slots'] == kmer._wanted_slots(info['windows'])
        assert name != 'F1' or info['slots'] < plain['slots']
        # --slots still overrides, and a device plane is served like a host plane
        import torch
        d = [torch.from_numpy(np.array(a)).cuda() for a in (f['seq'], f['qual'], f['meta'].view(np.int32))]
        dout, dinfo = kmer.correct_reads(d[0], d[2], k=f['k'], qual_plane=d[1], kmer_min_qual=f['Q'], slots=1 << 18)
        assert dinfo['slots'] == 1 << 18 and np.array_equal(dout.cpu().numpy(), f['out'])


def test_a_gate_that_leaves_no_window():
    from kbbq import kmer
    """The run ends as an empty table ends: solid_threshold of an all-zero histogram is 2, nothing is solid, nothing changes."""
    f = G.fixture('F1')
    empty = np.zeros(257, dtype=np.int64)
    for kw in ({}, dict(min_count=3)):
        out, info = kmer.correct_reads(f['seq'], f['meta'], k=f['k'], qual_plane=f['qual'], kmer_min_qual=93, **kw)
        assert info['counted_windows'] == 0 and info['windows'] == kmer.kmer_total(f['meta'], f['k']) and np.array_equal(info['hist'], empty)
        assert info['min_count'] == (kw.get('min_count') or kmer.solid_threshold(empty)) and np.array_equal(out, f['seq'])
        assert int(np.asarray(info['changed']).sum()) == 0


# ---------------------------------------------------------------- the commands
def _kbbq(*argv, timeout=300, env=None):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + [str(a) for a in argv], capture_output=True, timeout=timeout,
                          env=env or ENV)


def _said(stderr):
    """The commands' own lines of a stderr."""
    return ''.join(ln + '\n' for ln in stderr.decode().split('\n') if ln.startswith('kbbq '))


def _fastq_text(seq, qual, meta):
    lens = np.asarray(meta, dtype=np.int64) & 0xFFFF
    return ''.join('@r%d\n%s\n+\n%s\n' % (i, seq[i, :lens[i]].tobytes().decode(), qual[i, :lens[i]].tobytes().decode())
                   for i in range(seq.shape[0]))


@pytest.fixture(scope='module')
def fq(tmp_path_factory):
    f = G.fixture('F1')
    path = tmp_path_factory.mktemp('gate') / 'F1.fq'
    path.write_text(_fastq_text(f['seq'], f['qual'], f['meta']))
    return path


@pytest.mark.parametrize('more', ((), ('--prefilter', '--partitions', '3')))
def test_correct_command(fq, more):
    f = G.fixture('F1')
    G.assert_not_vacuous(f)
    gated = _kbbq('correct', '-f', fq, '-k', f['k'], '--kmer-min-qual', f['Q'], *more)
    plain = _kbbq('correct', '-f', fq, '-k', f['k'], *more)
    assert gated.returncode == 0 and plain.returncode == 0, (gated.stderr + plain.stderr).decode()[-3000:]
    assert gated.stdout.decode() == _fastq_text(f['out'], f['qual'], f['meta'])
    assert plain.stdout.decode() == _fastq_text(f['plain_out'], f['qual'], f['meta']) and gated.stdout != plain.stdout
    field = ' kmer_min_qual=%d counted_windows=%d' % (f['Q'], f['windows'])
    head = 'kbbq correct: k=%d min_count=%d reads=%d changed_bases=%d' % (f['k'], f['t'], f['seq'].shape[0], int(f['changed'].sum()))
    said = _said(gated.stderr)
    if more:
        assert re.fullmatch(re.escape(head + ' partitions=3' + field) + r' prefilter=1 admitted=\d+ slots=\d+\n', said), said
    else:
        assert said == head + field + '\n'
    assert 'kmer_min_qual' not in _said(plain.stderr) and _said(plain.stderr).startswith('kbbq correct: k=%d min_count=%d ' % (f['k'], f['plain_t']))


def _ok(*argv):
    r = _kbbq(*argv)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r


@pytest.mark.parametrize('opts', ((), ('--skip-unresolved', '--passes', '2')), ids=['plain', 'skip-passes'])
def test_recalibrate_c_is_correct_then_recalibrate_f(fq, tmp_path, opts):
    """`recalibrate -c reads --kmer-min-qual Q` is `correct --kmer-min-qual Q` followed by `recalibrate -f reads corrected`.  With
    --skip-unresolved the model of the two-file form is tallied from a reads file whose unresolved bases -- class 2 of the CPU
    model against the GATED count -- have the quality '!' (tests/test_gpu_recalibrate_skip.py has the argument)."""
    from kmer_skip_model import masked_quals
    f = G.fixture('F1')
    G.assert_not_vacuous(f)
    gate = ('-k', f['k'], '--kmer-min-qual', f['Q'])
    passes = ('--passes', '2') if opts else ()
    cor, m, m2 = tmp_path / 'cor.fq', tmp_path / 'm.txt', tmp_path / 'm2.txt'
    c = _ok('correct', '-f', fq, '-o', cor, *gate, *passes)
    said = _said(c.stderr)
    tallied = fq
    if opts:
        cls, t = G.classify(f['seq'], f['qual'], f['meta'], f['k'], f['Q'] + 33, passes=2)
        assert t == f['t'] and int((cls == 2).sum()) > 0
        tallied = tmp_path / 'masked.fq'
        tallied.write_text(_fastq_text(f['seq'], masked_quals(f['qual'], cls), f['meta']))
    _ok('recalibrate', '-f', tallied, cor, '-g', m)
    want = _ok('recalibrate', '-f', fq, cor, '-g', m).stdout
    got = _ok('recalibrate', '-c', fq, '-g', m2, *gate, *opts)
    assert len(want) > 0 and got.stdout == want and m2.read_bytes() == m.read_bytes()
    head = re.match(r'kbbq correct: (k=\d+ min_count=\d+ reads=\d+ changed_bases=\d+)( passes=2)? kmer_min_qual=', said)
    assert head and ('min_count=%d ' % f['t']) in said, said
    line = 'kbbq recalibrate: ' + head.group(1) + (' skipped_bases=%d passes=2' % int((cls == 2).sum()) if opts else '') \
        + ' kmer_min_qual=%d counted_windows=%d\n' % (f['Q'], f['windows'])
    assert _said(got.stderr) == line
    # ... and not what the command gives without the option
    plain = _ok('recalibrate', '-c', fq, '-k', f['k'], *opts)
    assert plain.stdout != got.stdout and 'kmer_min_qual' not in _said(plain.stderr)


# aligned records: the fixtures of tests/test_gpu_bqsr_mixed.py, one length and several
ALIGNED_K, ALIGNED_Q = 15, 4          # QUAL and OQ are uniform in 2..41: at Q = 4 about 0.95^15 of the windows are counted


def _flag_bits(i):
    return (0x800 if i % 7 == 0 else 0) | (0x400 if i % 11 == 0 else 0)


@pytest.fixture(scope='module')
def aligned(tmp_path_factory):
    import kmer_mixed_model as MX
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('gate_sam')
    paths = OQ.synth_bqsr_set(str(d), **MX.FIXTURE)
    whole = open(paths['sam']).read()
    out, idx = [], 0
    for ln in MX.shorten(whole, 'mixed').split('\n'):
        if ln and not ln.startswith('@'):
            fields = ln.split('\t')
            ln = '\t'.join(fields[:1] + [str(int(fields[1]) | _flag_bits(idx))] + fields[2:])
            idx += 1
        out.append(ln)
    marked = d / 'marked.sam'
    marked.write_text('\n'.join(out))
    fx = dict(paths=dict(paths, whole=paths['sam'], marked=str(marked)), mask=np.array([_flag_bits(i) != 0 for i in range(600)]))
    fx['whole'], fx['rgs'], fx['pus'] = MX.load(paths['sam'])
    fx['marked'] = MX.load(str(marked))[0]
    assert len(fx['marked']) == 600 and len({len(r.query_sequence) for r in fx['marked']}) > 1
    return fx


_aligned_memo = {}


def _aligned_model(fx, key, use_oq, masked):
    """(class plane, t, counted windows) of the gated model for a file of the fixture, computed once."""
    memo = (key, use_oq, masked)
    if memo not in _aligned_memo:
        _aligned_memo[memo] = G.aligned_classes(fx[key], ALIGNED_K, ALIGNED_Q, use_oq=use_oq, exclude=fx['mask'] if masked else None)
    return _aligned_memo[memo]


@pytest.mark.parametrize('key,opts,exclude', [('whole', ('-u',), ()), ('marked', ('--mixed-lengths',), ('-F', '0xF00'))],
                         ids=['one-length-u', 'mixed-F'])
def test_bqsr_and_recalibrate_b(aligned, tmp_path, key, opts, exclude):
    """`bqsr --kmers --kmer-min-qual Q` writes the model's report; `recalibrate -b --kmers --kmer-min-qual Q` is that command
    followed by `applybqsr`."""
    import kmer_mixed_model as MX
    from kbbq.gatk import bqsr
    use_oq, masked = '-u' in opts, bool(exclude)
    path = aligned['paths'][key]
    cls, t, counted = _aligned_model(aligned, key, use_oq, masked)
    assert 0 < counted and 0 < int((cls == 1).sum())
    want, winfo = MX.vectors(aligned[key], aligned['rgs'], ALIGNED_K, t, use_oq=use_oq, exclude=aligned['mask'] if masked else None,
                             flagged=(cls == 1, t))
    wanted, grp, grp2 = tmp_path / 'want.grp', tmp_path / 'R.grp', tmp_path / 'R2.grp'
    bqsr.vectors_to_report(*want, aligned['pus']).write(str(wanted))
    gate = ('--kmers', '-k', ALIGNED_K, '--kmer-min-qual', ALIGNED_Q, *opts, *exclude)
    first = _ok('bqsr', '-b', path, *gate, '-g', grp)
    assert first.stdout == b'' and grp.read_bytes() == wanted.read_bytes()
    tail = 'k=%d min_count=%d reads=600%s flagged_bases=%d kmer_min_qual=%d counted_windows=%d\n' % (
        ALIGNED_K, t, ' excluded_reads=%d' % int(aligned['mask'].sum()) if masked else '', winfo['flagged_bases'], ALIGNED_Q, counted)
    assert _said(first.stderr) == 'kbbq bqsr: ' + tail
    ungated = _ok('bqsr', '-b', path, '--kmers', '-k', ALIGNED_K, *opts, *exclude, '-g', tmp_path / 'plain.grp')
    assert (tmp_path / 'plain.grp').read_bytes() != grp.read_bytes() and 'kmer_min_qual' not in _said(ungated.stderr)
    second = _ok('applybqsr', '-b', path, '-g', grp, *[x for x in opts if x == '-u'])
    one = _ok('recalibrate', '-b', path, *gate, '-g', grp2)
    assert len(second.stdout) > 0 and one.stdout == second.stdout and grp2.read_bytes() == grp.read_bytes()
    assert _said(one.stderr) == 'kbbq recalibrate: ' + tail


def test_benchmark_command(aligned, tmp_path):
    import kmer_benchmark_model as KB
    p = aligned['paths']
    reads, ref, skips = KB.load(dict(p, sam=p['whole']))
    cls, t, counted = _aligned_model(aligned, 'whole', False, False)
    want, winfo = KB.joint(reads, ref, skips, ALIGNED_K, t, classified=(cls, t))
    assert want.sum(axis=0).min() >= 10
    base = ('benchmark', '-b', p['whole'], '-r', p['fa'], '-v', p['vcf'], '--kmers', '-k', ALIGNED_K, '-l', 'lbl')
    r = _ok(*base, '--kmer-min-qual', ALIGNED_Q)
    assert r.stdout.decode() == KB.render(want, 'lbl')
    assert _said(r.stderr) == KB.summary(winfo) + ' kmer_min_qual=%d counted_windows=%d\n' % (ALIGNED_Q, counted)
    plain = _ok(*base)
    assert plain.stdout != r.stdout and 'kmer_min_qual' not in _said(plain.stderr)
    # a record without qualities is refused by name before anything is uploaded
    from kbbq import aln, benchmark
    lines = open(p['whole']).read().split('\n')
    first = next(i for i, ln in enumerate(lines) if ln and not ln.startswith('@'))
    fields = lines[first + 4].split('\t')
    lines[first + 4] = '\t'.join(fields[:10] + ['*'] + fields[11:])
    bare = tmp_path / 'bare.sam'
    bare.write_text('\n'.join(lines))
    uploads = []
    real = benchmark._flag_batch
    benchmark._flag_batch = lambda *a, **kw: uploads.append(1) or real(*a, **kw)
    try:
        with pytest.raises(ValueError, match=r'record 4 \(%s\) has no qualities' % re.escape(fields[0])):
            benchmark.benchmark_kmers(aln.AlignmentFile(str(bare)), benchmark.get_ref_dict(p['fa']), benchmark.get_var_sites(p['vcf']),
                                      k=ALIGNED_K, kmer_min_qual=ALIGNED_Q)
    finally:
        benchmark._flag_batch = real
    assert not uploads


# ---------------------------------------------------------------- ranks
RANKS = 2


def test_two_ranks_write_the_one_process_bytes(fq, tmp_path):
    """`correct --kmer-min-qual` on 2 ranks sharing the GPU (tests/dist_kmer_gate_worker.py): every rank gates its own shard, the
    rank files concatenated are the one-process bytes -- the model's -- and counted_windows is the sum over the ranks."""
    import glob
    import json
    import socket
    f = G.fixture('F1')
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / 'out.fq')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
    env.setdefault('KBBQ_DIST_BACKEND', 'gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(RANKS), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(ROOT, 'tests', 'dist_kmer_gate_worker.py'), str(fq), str(f['k']), str(f['Q']), out]
    r = subprocess.run(cmd, env=env, capture_output=True, timeout=400)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    parts = sorted(glob.glob(out + '.rank????'))
    assert len(parts) == RANKS
    assert b''.join(open(p, 'rb').read() for p in parts).decode() == _fastq_text(f['out'], f['qual'], f['meta'])
    infos = [json.load(open(p + '.json')) for p in parts]
    assert all(i['mine'] > 0 for i in infos) and sum(i['mine'] for i in infos) == f['windows']
    assert sum(i['reads_mine'] for i in infos) == f['seq'].shape[0]
    for i in infos:
        assert (i['counted_windows'], i['min_count'], i['kmer_min_qual'], i['reads']) == (f['windows'], f['t'], f['Q'], f['seq'].shape[0])
    assert _said(r.stderr) == 'kbbq correct: k=%d min_count=%d reads=%d changed_bases=%d kmer_min_qual=%d counted_windows=%d\n' % (
        f['k'], f['t'], f['seq'].shape[0], int(f['changed'].sum()), f['Q'], f['windows'])
