"""`--partitions P` on the MI355X: the two partition count kernels against the CPU model of one partition
(tests/kmer_partition_model.py), from device planes, host planes and device batches in the recalibrate path's layouts; the
edges (empty partitions, a row of more than 256 chunks, breaks, parts == 1); the whole rule (kbbq.kmer.correct_reads with
partitions against partitions=1 and the CPU models) with and without the prefilter, the N rule and several passes; a table the
whole input does not fit and one partition does; `auto` under a device budget; and the four commands, each in a child process
against the same command without the option."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmer_model as M
import kmer_partition_model as PT
import kmer_passes_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_SEQUENTIAL', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_DEVICE_BUDGET', 'KBBQ_TALLY_FUSED'):
    ENV.pop(_var, None)

MODEL_ROWS = 128                      # rows of F whose corrected bytes the CPU model of the rule is run on (it walks bases in Python)
_memo = {}


@pytest.fixture(scope='module')
def F():
    """F on the host and on the device."""
    import torch
    seq, meta = PT.fixture()
    return dict(seq=seq, meta=meta, d_seq=torch.from_numpy(np.array(seq)).cuda(),
                d_meta=torch.from_numpy(np.array(meta).view(np.int32)).cuda())


def _entries(table):
    keys, counts = table.entries()
    table.close()
    return keys, counts.astype(np.int64)


def _same_pairs(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- the kernels against the model
@pytest.mark.parametrize('k', (15, 31, 32))
@pytest.mark.parametrize('P, p', ((2, 0), (3, 2), (64, 17)))
def test_one_partition_is_the_models(F, k, P, p):
    from kbbq import kmer
    keys, counts = PT.counted(k)
    want = PT.partition(keys, counts, P, p)
    assert 0 < want[0].size < keys.size
    _same_pairs(_entries(kmer.count_kmers(F['d_seq'], F['d_meta'], k=k, parts=P, part=p)), want)


@pytest.mark.parametrize('source', ('device', 'host'))
def test_all_partitions_into_one_table_are_one_count(F, source):
    from kbbq import kmer
    k = 31
    keys, counts = PT.counted(k)
    seq, meta = (F['d_seq'], F['d_meta']) if source == 'device' else (F['seq'], F['meta'])
    table = kmer.count_kmers(seq, meta, k=k, parts=3, part=1)
    gk, gc = table.entries()
    _same_pairs((gk, gc.astype(np.int64)), PT.partition(keys, counts, 3, 1))
    for p in (2, 0):
        kmer.count_kmers(seq, meta, table=table, parts=3, part=p)
    _same_pairs(_entries(table), (keys, counts))


def test_filtered_partitions(F):
    """The filtered kernel: every partition holds its keys of count >= 2 exactly and of the once-seen keys only its own."""
    from kbbq import kmer
    k = 21
    keys, counts = PT.counted(k)
    for source in ('device', 'host'):
        seq, meta = (F['d_seq'], F['d_meta']) if source == 'device' else (F['seq'], F['meta'])
        filt = kmer.prefilter_kmers(seq, meta, k=k)
        filt.release_seen()
        whole = _entries(kmer.count_kmers(seq, meta, k=k, filter=filt, slots=1 << 18))
        got_keys, got_counts = [], []
        for p in range(3):
            gk, gc = _entries(kmer.count_kmers(seq, meta, k=k, filter=filt, slots=1 << 17, parts=3, part=p))
            assert (PT.part(gk, 3) == p).all()
            wk, wc = PT.partition(keys, counts, 3, p)
            twice = gc >= 2
            assert np.array_equal(gk[twice], wk[wc >= 2]) and np.array_equal(gc[twice], wc[wc >= 2])
            got_keys.append(gk)
            got_counts.append(gc)
        filt.close()
        gk, gc = np.concatenate(got_keys), np.concatenate(got_counts)
        order = np.argsort(gk, kind='stable')
        _same_pairs((gk[order], gc[order]), whole)                         # the same filter admits the same singletons


def _rows_module():
    import test_gpu_kmer_rows as R
    return R


@pytest.mark.parametrize('layout', ('reads_nib', 'pairs_nib', 'twins', 'reads'))
def test_partitions_of_device_batches(layout):
    """count_batch on the batches tests/test_gpu_kmer_rows.py builds: 4-bit planes, two reads to a row, character rows."""
    from kbbq import _device as dev
    from kbbq import kmer
    R = _rows_module()
    k = 21
    if layout in ('reads_nib', 'reads'):
        seq, meta = M.synth(11, genome_len=5000, depth=30, err=0.01, len_lo=36, len_hi=300)[:2]
        batch = R._batch(seq, meta)
        laid = dev.lay_out(batch, 1) if layout == 'reads_nib' else batch
    elif layout == 'pairs_nib':
        laid = dev.lay_out(R._batch(*R._fixed(70, 50)), 1)
    else:
        seq, meta = R._fixed(31, 100, paired=False)
        laid = dev.lay_out(R._batch(seq[:-1], meta[:-1]), 1)
        assert laid.twins
    assert laid.layout_key() == ('pairs_nib' if layout == 'twins' else layout)
    chars, lens = R._rows(laid)
    keys, counts = M.count(chars, lens, k)
    for P, p in ((2, 1), (64, 40)):
        _same_pairs(_entries(kmer.count_batch(laid, k=k, parts=P, part=p)), PT.partition(keys, counts, P, p))
    table = kmer.count_batch(laid, k=k, parts=3, part=0)
    for p in (1, 2):
        kmer.count_batch(laid, table=table, parts=3, part=p)
    _same_pairs(_entries(table), (keys, counts))
    # ... and the filtered form on the same rows
    filt = kmer.prefilter_batch(laid, k)
    filt.release_seen()
    hist = np.zeros(kmer.HIST, dtype=np.int64)
    for p in range(3):
        t = kmer.count_batch(laid, k=k, filter=filt, parts=3, part=p)
        hist += kmer.kmer_histogram(t)
        gk, gc = _entries(t)
        wk, wc = PT.partition(keys, counts, 3, p)
        assert np.array_equal(gk[gc >= 2], wk[wc >= 2]) and np.array_equal(gc[gc >= 2], wc[wc >= 2])
    filt.close()
    assert np.array_equal(hist[2:], M.histogram(counts)[2:])


# ---------------------------------------------------------------- edges
def test_four_short_reads_in_64_partitions():
    from kbbq import kmer
    rng = np.random.default_rng(21)
    a, b = (bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, 40)]) for _ in range(2))
    seq, meta = M.plane([a, b, a, b[:39] + (b'A' if b[39:] != b'A' else b'C')])
    keys, counts = M.count(seq, meta, 31)
    assert keys.size <= 40 and int((counts >= 2).sum()) >= 10
    empty = 64 - np.unique(PT.part(keys, 64)).size
    assert empty > 24                                     # most partitions hold no key at all
    one, info1 = kmer.correct_reads(seq, meta, k=31, min_count=2)
    got, info = kmer.correct_reads(seq, meta, k=31, min_count=2, partitions=64)
    assert np.array_equal(got, one) and np.array_equal(info['changed'], info1['changed']) and np.array_equal(info['hist'], info1['hist'])
    assert np.array_equal(info['hist'], M.histogram(counts))
    assert info['partitions'] == 64 and info['kept_pairs'] == int((counts >= 2).sum()) and info['min_count'] == 2
    # a partition without a key: nothing is counted and select returns nothing
    p = int(np.setdiff1d(np.arange(64), PT.part(keys, 64))[0])
    table = kmer.count_kmers(seq, meta, k=31, parts=64, part=p)
    sel = kmer.select(table, 1, 1)
    assert int(sel[0].shape[0]) == 0 and int(sel[2].sum()) == 0 and table.entries()[0].size == 0
    table.close()


def test_a_row_of_more_than_256_chunks():
    import torch
    from kbbq import kmer
    rng = np.random.default_rng(22)
    read = bytes(np.frombuffer(M.LETTERS, dtype=np.uint8)[rng.integers(0, 4, 5000)])
    seq, meta = M.plane([read, read[100:4000], read[:33]])
    assert seq.shape[1] // 16 == 313                      # one row a workgroup
    keys, counts = M.count(seq, meta, 31)
    d_seq, d_meta = torch.from_numpy(seq).cuda(), torch.from_numpy(meta.view(np.int32)).cuda()
    _same_pairs(_entries(kmer.count_kmers(d_seq, d_meta, k=31, parts=8, part=5)), PT.partition(keys, counts, 8, 5))
    table = kmer.count_kmers(d_seq, d_meta, k=31, parts=2, part=1)
    kmer.count_kmers(d_seq, d_meta, table=table, parts=2, part=0)
    _same_pairs(_entries(table), (keys, counts))


def test_breaks(F):
    import torch
    from kbbq import kmer
    seq, meta = np.array(F['seq'][:400]), np.array(F['meta'][:400])
    rng = np.random.default_rng(23)
    inside = np.arange(seq.shape[1])[None, :] < meta.astype(np.int64)[:, None]
    low = inside & (rng.random(seq.shape) < 0.01)
    seq[low] |= 0x20
    seq[inside & (rng.random(seq.shape) < 0.005)] = ord('N')
    assert (seq == ord('N'))[inside].any() and np.isin(seq, np.frombuffer(b'acgt', dtype=np.uint8)).any()
    keys, counts = M.count(seq, meta, 15)
    assert keys.size < M.count(F['seq'][:400], F['meta'][:400], 15)[0].size
    d_seq, d_meta = torch.from_numpy(seq).cuda(), torch.from_numpy(meta.view(np.int32)).cuda()
    for P, p in ((2, 1), (3, 0)):
        _same_pairs(_entries(kmer.count_kmers(d_seq, d_meta, k=15, parts=P, part=p)), PT.partition(keys, counts, P, p))
        _same_pairs(_entries(kmer.count_kmers(seq, meta, k=15, parts=P, part=p)), PT.partition(keys, counts, P, p))


def test_parts_1_is_the_call_without(F):
    from kbbq import _native as N
    from kbbq import kmer
    lib = N.load()
    d_seq, d_meta = F['d_seq'], F['d_meta']
    n, pitch = d_seq.shape
    want = _entries(kmer.count_kmers(d_seq, d_meta, k=31))
    _same_pairs(want, PT.counted(31))
    table = kmer.KmerTable(31, 1 << 19)
    N.check(lib.kbbq_kmer_count_part_dev(table.ctx.handle, table.handle, N.ptr(d_seq), N.ptr(d_meta), n, pitch, 1, 0))
    table.ctx.status()
    _same_pairs(_entries(table), want)
    table = kmer.KmerTable(31, 1 << 19)
    N.check(lib.kbbq_kmer_count_rows_part_dev(table.ctx.handle, table.handle, N.ptr(d_seq), N.ptr(d_meta), n, pitch, 0, 1, 0))
    table.ctx.status()
    _same_pairs(_entries(table), want)
    table = kmer.KmerTable(31, 1 << 19)
    seq, meta = np.ascontiguousarray(F['seq']), np.ascontiguousarray(F['meta'])
    N.check(lib.kbbq_kmer_count_part(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, 1, 0))
    _same_pairs(_entries(table), want)


# ---------------------------------------------------------------- the whole rule
VARIANTS = {'plain': {}, 'prefilter': dict(prefilter=True), 'fix_n': dict(fix_n=True), 'passes': dict(passes=3)}


def _one_table(F, k, variant):
    """correct_reads(F, partitions=1) for a variant, once."""
    from kbbq import kmer
    key = ('one', k, variant)
    if key not in _memo:
        out, info = kmer.correct_reads(F['d_seq'], F['d_meta'], k=k, **VARIANTS[variant])
        _memo[key] = (out.cpu().numpy(), np.asarray(info['changed'].cpu().numpy()), info)
    return _memo[key]


def _model_rows(F, k, variant):
    """The CPU model's corrected bytes of the first MODEL_ROWS rows of F against the solid set of all of F, once.  The
    prefilter does not change the rule's inputs (solid keys), so its model is the plain one."""
    kw = {key: v for key, v in VARIANTS[variant].items() if key != 'prefilter'}
    key = ('model', k, tuple(sorted(kw.items())))
    if key not in _memo:
        keys, counts = PT.counted(k)
        t = PT.FIGURES[k][3]
        plane, changed = PM.passes(F['seq'][:MODEL_ROWS], F['meta'][:MODEL_ROWS], k, t, kw.get('passes', 1), fix_n=kw.get('fix_n', False),
                                   solid_keys=keys[counts >= t])[:2]
        _memo[key] = (plane, changed)
    return _memo[key]


@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('P', (2, 3, 8))
@pytest.mark.parametrize('k', (21, 31))
def test_correct_reads_in_partitions_is_correct_reads(F, k, P, variant):
    from kbbq import kmer
    one, one_changed, one_info = _one_table(F, k, variant)
    out, info = kmer.correct_reads(F['d_seq'], F['d_meta'], k=k, partitions=P, **VARIANTS[variant])
    got, changed = out.cpu().numpy(), info['changed'].cpu().numpy()
    assert np.array_equal(got, one) and np.array_equal(changed, one_changed) and int(changed.sum()) > 0
    assert info['min_count'] == one_info['min_count'] == PT.FIGURES[k][3]
    keys, counts = PT.counted(k)
    lo = 2 if variant == 'prefilter' else 0
    assert np.array_equal(info['hist'][lo:], one_info['hist'][lo:]) and np.array_equal(info['hist'][lo:], M.histogram(counts)[lo:])
    assert info['partitions'] == P and info['kept_pairs'] == PT.FIGURES[k][2]
    total = info['admitted'] if variant == 'prefilter' else PT.FIGURES[k][0]
    assert info['slots'] == kmer.default_slots(kmer.partition_windows(total, P), 1 << 40) and info['table_bytes'] == 12 * info['slots']
    assert info['solid_slots'] == kmer.default_slots(info['kept_pairs'], 1 << 40)
    want, want_changed = _model_rows(F, k, variant)
    assert np.array_equal(got[:MODEL_ROWS], want) and np.array_equal(changed[:MODEL_ROWS].astype(np.int64), want_changed)


def test_min_count_given_keeps_from_min_count(F):
    from kbbq import kmer
    keys, counts = PT.counted(31)
    one = kmer.correct_reads(F['d_seq'], F['d_meta'], k=31, min_count=7)
    got = kmer.correct_reads(F['d_seq'], F['d_meta'], k=31, min_count=7, partitions=3)
    assert np.array_equal(got[0].cpu().numpy(), one[0].cpu().numpy()) and got[1]['min_count'] == 7
    assert got[1]['kept_pairs'] == int((counts >= 7).sum())
    with pytest.raises(ValueError, match='min_count must be >= 1'):
        kmer.correct_reads(F['d_seq'], F['d_meta'], k=31, min_count=0, partitions=3)


@pytest.mark.parametrize('passes', (1, 2))
def test_flags_against_the_solid_table(F, passes):
    from kbbq import _device as dev
    from kbbq import kmer
    k, P = 31, 3
    d_seq, d_meta = F['d_seq'], F['d_meta']
    budget = dev.device_budget()
    solid, hist, t, info = kmer.count_partitioned(lambda tab, p: kmer.count_kmers(d_seq, d_meta, k=k, table=tab, parts=P, part=p), k, P,
                                                  kmer.partition_slots(PT.FIGURES[k][0], P, budget), None, budget)
    full = kmer.count_kmers(d_seq, d_meta, k=k)
    try:
        assert t == PT.FIGURES[k][3] and np.array_equal(hist, kmer.kmer_histogram(full))
        keys, counts = PT.counted(k)
        sk, sc = solid.entries()
        assert np.array_equal(sk, keys[counts >= 2]) and np.array_equal(sc.astype(np.int64), counts[counts >= 2])   # all kept pairs are merged
        more = kmer._passes_kw(passes)
        got = kmer.flag_errors(solid, d_seq, d_meta, t, unresolved=True, **more)
        want = kmer.flag_errors(full, d_seq, d_meta, t, unresolved=True, **more)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w.cpu().numpy())
        assert int((got[0] == 2).sum().item()) > 0 and int((got[0] == 1).sum().item()) > 0
    finally:
        solid.close()
        full.close()


# ---------------------------------------------------------------- the ceiling moves
def test_a_table_the_input_does_not_fit_and_a_partition_does(F):
    from kbbq import _native as N
    from kbbq import kmer
    one, one_changed, one_info = _one_table(F, 31, 'plain')
    assert PT.FIGURES[31][1] > 1 << 16                    # 144,905 keys do not fit 65,536 slots
    with pytest.raises(N.KmerTableFull, match=r'slots=65536 is too small for these reads: give more slots'):
        kmer.correct_reads(F['d_seq'], F['d_meta'], k=31, slots=1 << 16, partitions=1)
    out, info = kmer.correct_reads(F['d_seq'], F['d_meta'], k=31, slots=1 << 16, partitions=8)
    assert np.array_equal(out.cpu().numpy(), one) and np.array_equal(info['changed'].cpu().numpy(), one_changed)
    assert info['slots'] == 1 << 16 and info['table_bytes'] == 12 << 16 and info['kept_pairs'] == 22594 == PT.FIGURES[31][2]
    assert PT.LARGEST[31][8] / (1 << 16) < 0.28 + 0.005   # the largest partition loads the table to 0.28
    # a partition round that fills keeps today's text
    with pytest.raises(N.KmerTableFull, match=r'slots=16384 is too small for these reads: give more slots'):
        kmer.correct_reads(F['d_seq'], F['d_meta'], k=31, slots=1 << 14, partitions=8)
    out, _ = kmer.correct_reads(F['d_seq'], F['d_meta'], k=31, partitions=2)      # the context goes on working
    assert np.array_equal(out.cpu().numpy(), one)


# ---------------------------------------------------------------- the commands
def _kbbq(*argv, timeout=300, env=None):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + [str(a) for a in argv], capture_output=True, timeout=timeout,
                          env=env or ENV)


def _said(stderr):
    """The commands' own lines of a stderr."""
    return ''.join(ln + '\n' for ln in stderr.decode().split('\n') if ln.startswith('kbbq '))


PARTS = re.compile(r' partitions=(\d+)')
PREFILTER = re.compile(r' prefilter=1 admitted=\d+ slots=\d+')


def _pair(argv, option, out=None, tmp=None, prefilter=False):
    """The command with and without `option`; -> (with, without, P printed).  stdout and the file `out` names (given as a
    placeholder '{out}' in argv) byte-equal, stderr equal without ` partitions=P` (and, with the prefilter, without its group:
    `admitted` depends on the order of the filter's atomics, and `slots` describes the per-partition table)."""
    res = []
    for i, more in enumerate(((), option)):
        path = tmp / ('out%d' % i) if out else None
        r = _kbbq(*[str(a).replace('{out}', str(path)) for a in argv], *more)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        res.append((r, path.read_bytes() if out else b''))
    (plain, plain_file), (parted, parted_file) = res
    assert parted.stdout == plain.stdout and parted_file == plain_file and len(plain.stdout) + len(plain_file) > 0
    err, perr = _said(plain.stderr), _said(parted.stderr)
    assert err
    found = PARTS.findall(perr)
    assert not PARTS.search(err) and len(found) == 1, perr
    if prefilter:
        assert len(PREFILTER.findall(err)) == len(PREFILTER.findall(perr)) == 1
        assert perr.rstrip('\n').endswith(PREFILTER.search(perr).group(0))        # the group stays last
        assert PREFILTER.sub('', PARTS.sub('', perr)) == PREFILTER.sub('', err)
        assert re.search(r' partitions=\d+ prefilter=1 ', perr)
    else:
        assert PARTS.sub('', perr) == err
        assert re.search(r' partitions=\d+$', perr, flags=re.M)
    return parted, plain, int(found[0])


def _fastq(path, seq, meta, names=None):
    lens = np.asarray(meta, dtype=np.int64) & 0xFFFF
    qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    path.write_bytes(''.join('@%s\n%s\n+\n%s\n' % (names[i] if names else 'r%d' % i, seq[i, :lens[i]].tobytes().decode(),
                                                    qual[i, :lens[i]].tobytes().decode()) for i in range(seq.shape[0])).encode())
    return path


@pytest.fixture(scope='module')
def fq(F, tmp_path_factory):
    return _fastq(tmp_path_factory.mktemp('partitions') / 'F.fq', F['seq'], F['meta'])


@pytest.mark.parametrize('more', ((), ('--prefilter',), ('--fix-n', '--passes', '2', '--min-count', '4')))
def test_correct_command(F, fq, tmp_path, more):
    parted, plain, P = _pair(('correct', '-f', fq, *more), ('--partitions', '3'), tmp=tmp_path, prefilter='--prefilter' in more)
    assert P == 3
    if not more:
        one = _one_table(F, 31, 'plain')[0]
        lens = F['meta'].astype(np.int64)
        assert parted.stdout.decode().split('\n')[1::4][:50] == [one[i, :lens[i]].tobytes().decode() for i in range(50)]


def test_correct_auto_under_a_budget(F, fq, tmp_path):
    """The budget is one byte short of twice the one-table default of F's windows, so `auto` must split; P is the smallest number
    of partitions whose table -- ceil(windows x 9 / (8 P)) keys at a load factor of 0.5, a power of two, 12 bytes a slot -- fits
    half of it."""
    from kbbq import kmer
    windows = kmer.kmer_total(F['meta'], 31)

    def table_bytes(keys):
        slots = 1024
        while slots < 2 * keys:
            slots *= 2
        return 12 * slots
    budget = 2 * table_bytes(windows) - 1
    want = next(P for P in range(2, 65) if table_bytes(-(-windows * 9 // (8 * P))) <= budget // 2)
    assert want > 1 and budget > 1 << 20
    plain = _kbbq('correct', '-f', fq)
    r = _kbbq('correct', '-f', fq, '--partitions', 'auto', env=dict(ENV, KBBQ_DEVICE_BUDGET=str(budget)))
    assert plain.returncode == 0 and r.returncode == 0, (plain.stderr + r.stderr).decode()[-3000:]
    assert r.stdout == plain.stdout and len(r.stdout) > 0
    assert _said(plain.stderr) and _said(r.stderr) == _said(plain.stderr).rstrip('\n') + ' partitions=%d\n' % want
    # ... and where one table fits, auto is no option at all
    roomy = _kbbq('correct', '-f', fq, '--partitions', 'auto', env=dict(ENV, KBBQ_DEVICE_BUDGET=str(budget + 1)))
    assert roomy.returncode == 0 and roomy.stdout == plain.stdout and _said(roomy.stderr) == _said(plain.stderr)


def _two_bands(tmp, letter=None):
    """A FASTQ of two length bands (100 and 150 bases, shortest first) with read groups in the names; `letter`: one base of a
    read of the second band becomes that letter."""
    a, ma = M.synth(5, genome_len=3000, depth=30, err=0.01, len_lo=100, len_hi=100)[:2]
    b, mb = M.synth(6, genome_len=3000, depth=30, err=0.01, len_lo=150, len_hi=150)[:2]
    seq = np.full((a.shape[0] + b.shape[0], b.shape[1]), ord('N'), dtype=np.uint8)
    seq[:a.shape[0], :a.shape[1]] = a
    seq[a.shape[0]:] = b
    meta = np.concatenate([ma, mb])
    if letter:
        seq[a.shape[0] + 7, 60] = ord(letter)
    names = ['r%d_RG:Z:g%d' % (i, i % 3) for i in range(seq.shape[0])]
    return _fastq(tmp / ('bands%s.fq' % (letter or '')), seq, meta, names)


@pytest.mark.parametrize('more', ((), ('--skip-unresolved', '--passes', '2'), ('--prefilter',)))
def test_recalibrate_command(tmp_path, more):
    reads = _two_bands(tmp_path)
    _pair(('recalibrate', '-c', reads, '--infer-rg', '-g', '{out}', *more), ('--partitions', '3'), out=True, tmp=tmp_path,
          prefilter='--prefilter' in more)


def test_recalibrate_command_with_a_letter_outside_acgtn(tmp_path):
    """A band with a letter outside ACGTN is redone as character rows, which are corrected against the table still held -- with
    the option the solid table -- before the row-per-read tally refuses the read as the two-file form does.  The command ends as
    it ends without the option: the same status, the same exception, nothing on stdout."""
    reads = _two_bands(tmp_path, 'R')

    def raised(r):
        last = [x for x in r.stderr.decode().splitlines() if re.match(r'[A-Za-z_.]*(Error|Exception)\b', x)]
        return last[-1] if last else None
    plain = _kbbq('recalibrate', '-c', reads, '--infer-rg', '--skip-unresolved')
    parted = _kbbq('recalibrate', '-c', reads, '--infer-rg', '--skip-unresolved', '--partitions', '3')
    assert parted.returncode == plain.returncode and parted.stdout == plain.stdout
    assert raised(parted) == raised(plain) and (plain.returncode == 0) == (raised(plain) is None)
    assert PARTS.sub('', _said(parted.stderr)) == _said(plain.stderr)
    assert 'KmerTableFull' not in parted.stderr.decode() and 'partition' not in (raised(parted) or '')


def test_bands_redone_in_character_rows_meet_the_solid_table(tmp_path, monkeypatch):
    """In process, with input the tally accepts: a stand-in for K1's launcher refuses every band's own layout, so each band is
    redone one character row per read and corrected by the character kernels against the table held until the tally is over.
    With partitions that is the solid table: output, report and figures are those of the run without the option."""
    from kbbq import _device as dev
    from kbbq import recalibrate
    reads = _two_bands(tmp_path)

    def run(tag, **kw):
        out, report = tmp_path / (tag + '.fq'), tmp_path / (tag + '.txt')
        info = recalibrate.recalibrate_corrected(str(reads), infer_rg=True, output=str(out), gatkreport=str(report), **kw)
        return info, out.read_bytes(), report.read_bytes()
    laid = run('laid', skip_unresolved=True, passes=2)
    refused = []
    real = dev.accumulate

    def accumulate(batch, *args, **kw):
        if batch.nib or isinstance(batch, dev.PairBatch) or batch.seg is not None:
            refused.append(batch.layout_key())
            raise ValueError('a layout the tally does not serve (the test says so)')
        return real(batch, *args, **kw)

    def accumulate_bands(*args, **kw):
        raise ValueError('no merged launch (the test says so)')
    monkeypatch.setattr(dev, 'accumulate', accumulate)
    monkeypatch.setattr(dev, 'accumulate_bands', accumulate_bands)
    redone = run('redone', skip_unresolved=True, passes=2, partitions=3)
    assert len(refused) >= 2                                 # both length bands went the other way
    assert redone[1] == laid[1] and redone[2] == laid[2] and len(laid[1]) > 0 and len(laid[2]) > 0
    for key in ('min_count', 'reads', 'changed_bases', 'skipped_bases'):
        assert redone[0][key] == laid[0][key]
    assert np.array_equal(redone[0]['hist'], laid[0]['hist'])
    assert redone[0]['partitions'] == 3 and 'partitions' not in laid[0] and redone[0]['changed_bases'] > 0


@pytest.fixture(scope='module')
def aligned(tmp_path_factory):
    import kmer_bqsr_model as B
    import oracle_bqsr as OQ
    return OQ.synth_bqsr_set(str(tmp_path_factory.mktemp('partitions_sam')), **B.FIXTURE)


@pytest.mark.parametrize('more', ((), ('--skip-unresolved',), ('--prefilter', '-u')))
def test_bqsr_command(aligned, tmp_path, more):
    _pair(('bqsr', '-b', aligned['sam'], '--kmers', '-k', '15', '-g', '{out}', *more), ('--partitions', '3'), out=True, tmp=tmp_path,
          prefilter='--prefilter' in more)


def test_benchmark_command(aligned, tmp_path):
    _pair(('benchmark', '-b', aligned['sam'], '-r', aligned['fa'], '-v', aligned['vcf'], '--kmers', '-k', '15', '-l', 'lbl'),
          ('--partitions', '3'), tmp=tmp_path)
