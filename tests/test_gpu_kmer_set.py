"""K-mer sets on the MI355X: the bytes `kbbq count` writes against the format's CPU model (tests/kmer_set_model.py) -- every k and
keep, with the prefilter, in partitions, through the smallest table that fits, from split files, gated, from alignments, with
records left out --; the unsigned order of k = 32 keys; the sizes at the sort's and the check's edges and loads through several
slabs; every tampering the device check must find; and the five commands with --kmers-from against themselves without it."""
import os
import re
import sys

import numpy as np
import pytest

import kmer_gate_model as G
import kmer_model as M
import kmer_set_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = np.frombuffer(M.LETTERS, dtype=np.uint8)
_memo = {}


def _records(seq, qual, meta):
    lens = np.asarray(meta).astype(np.int64) & 0xFFFF
    return [(seq[i, :lens[i]].tobytes(), qual[i, :lens[i]].tobytes()) for i in range(seq.shape[0])]


def _fastq(path, records, first=0):
    with open(path, 'wb') as fh:
        for i, (s, q) in enumerate(records):
            fh.write(b'@r%d\n%s\n+\n%s\n' % (first + i, s, q))
    return str(path)


def _sam(path, records, flags=None):
    """A SAM file of the records as given (SEQ and QUAL as they are): one contig, one read group."""
    with open(path, 'wb') as fh:
        fh.write(b'@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:5000\n@RG\tID:g1\tPU:u1\n')
        for i, (s, q) in enumerate(records):
            fh.write(b'a%d\t%d\tchr1\t%d\t60\t%dM\t*\t0\t0\t%s\t%s\tRG:Z:g1\n' % (i, 0 if flags is None else flags[i], 1 + i % 1000, len(s), s, q))
    return str(path)


@pytest.fixture(scope='module')
def X(tmp_path_factory):
    """X: reads of 40..70 bases from both strands of a 2 kb genome at about 30x with 1 % substitutions, Ns, a lower-case base and
    reads shorter than every k, shortest first; as one FASTQ file, as two cut at a read boundary, and (upper case) as SAM."""
    d = tmp_path_factory.mktemp('kmer_set')
    seq, meta = M.synth(23, genome_len=2000, depth=30, err=0.01, len_lo=40, len_hi=70, n_rate=0.002)[:2]
    seq = seq.copy()
    seq[3, 20] = ord('a') if seq[3, 20] != ord('N') else ord('c')
    short = [b'ACGTA', b'ACGTACGTACGTACG'[:7], b'G' * 31]
    rows = [(seq[i, :int(meta[i])].tobytes()) for i in range(seq.shape[0])] + short
    rows.sort(key=len)
    seq, meta = M.plane(rows)
    qual = G.quals(seq, meta)
    records = _records(seq, qual, meta)
    assert any(b'N' in s for s, _ in records) and any(b'a' in s or b'c' in s for s, _ in records) and len(records[0][0]) == 5
    cut = len(records) // 3
    upper = [(s.upper(), q) for s, q in records]
    flags = [0x400 if i % 7 == 3 else (16 if i % 2 else 0) for i in range(len(records))]
    return dict(dir=d, records=records, seq=seq, qual=qual, meta=meta, fq=_fastq(d / 'x.fq', records),
                fq1=_fastq(d / 'x1.fq', records[:cut]), fq2=_fastq(d / 'x2.fq', records[cut:], cut), upper=upper, flags=flags,
                sam=_sam(d / 'x.sam', upper, flags), sam2=_sam(d / 'x2.sam', upper[cut:]), fq1u=_fastq(d / 'x1u.fq', upper[:cut]),
                long=[r for r in upper if len(r[0]) >= 40], fqlong=_fastq(d / 'long.fq', [r for r in upper if len(r[0]) >= 40]))


def _want(records, k, keep, Q=None, reads=None, tag='X'):
    key = (tag, k, keep, Q, reads)
    if key not in _memo:
        _memo[key] = SM.set_bytes(records, k, keep, Q, reads)
    return _memo[key]


def _count(tmp_path, name, *inputs, **kw):
    from kbbq import kmerset
    out = str(tmp_path / name)
    info = kmerset.count(*inputs, output=out, **kw)
    with open(out, 'rb') as fh:
        return fh.read(), info, out


# ---------------------------------------------------------------- 1. bytes
@pytest.mark.parametrize('keep', (1, 2, 3))
@pytest.mark.parametrize('k', (8, 15, 31, 32))
def test_count_writes_the_models_bytes(X, tmp_path, k, keep):
    want = _want(X['records'], k, keep)
    f = SM.parse(want)
    assert f['n'] > 50 and f['windows'] > f['n'] and SM.check_pairs(f['keys'], f['counts'], k, keep, f['key_sum'], f['count_sum']) is None
    got, info, _ = _count(tmp_path, 'plain.set', [X['fq']], k=k, keep=keep)
    assert got == want
    total = int(np.maximum(X['meta'].astype(np.int64) - k + 1, 0).sum())             # every window, the broken ones too
    assert (info['kmers'], info['reads'], info['counted_windows'], info['inputs']) == (f['n'], len(X['records']), f['windows'], 1)
    assert info['windows'] == total > f['windows']
    # the same bytes in three rounds, from two files cut at a read boundary, and (keep >= 2) behind the prefilter
    assert _count(tmp_path, 'parts.set', [X['fq']], k=k, keep=keep, partitions=3)[0] == want
    got, info, _ = _count(tmp_path, 'split.set', [X['fq1'], X['fq2']], k=k, keep=keep, slab=100)
    assert got == want and info['inputs'] == 2
    if keep >= 2:
        got, info, _ = _count(tmp_path, 'pre.set', [X['fq1'], X['fq2']], k=k, keep=keep, prefilter=True, partitions=2)
        assert got == want and info['admitted'] > 0 and info['partitions'] == 2


def test_the_smallest_table_that_fits_writes_the_same_bytes(X, tmp_path):
    from kbbq import _native as N
    k, keep = 15, 2
    want = _want(X['records'], k, keep)
    distinct = SM.count(X['records'], k)[0].size
    slots = 1024
    while slots < distinct:
        slots *= 2
    tried = []
    while True:                                  # a table that is too small is an ordinary error return and leaves no file
        tried.append(slots)
        try:
            got, info, _ = _count(tmp_path, 'min.set', [X['fq']], k=k, keep=keep, slots=slots)
            break
        except N.KmerTableFull:
            assert not os.path.exists(str(tmp_path / 'min.set')) and slots < 4 * distinct
            slots *= 2
    assert got == want and info['slots'] == slots and slots < 2 * distinct * 2, tried


@pytest.mark.parametrize('k', (15, 31))
def test_the_gate_and_the_histogram_file(X, tmp_path, k):
    want = _want(X['records'], k, 2, Q=20)
    f, plain = SM.parse(want), SM.parse(_want(X['records'], k, 2))
    assert 0 < f['n'] < plain['n'] and f['windows'] < plain['windows'] and f['min_qual'] == 20
    histo = str(tmp_path / 'h.tsv')
    got, info, _ = _count(tmp_path, 'gate.set', [X['fq1'], X['fq2']], k=k, kmer_min_qual=20, histo=histo)
    assert got == want and info['counted_windows'] == f['windows'] and info['windows'] > plain['windows']
    assert _count(tmp_path, 'gate_pre.set', [X['fq']], k=k, kmer_min_qual=20, prefilter=True, partitions=3)[0] == want
    assert open(histo).read() == ''.join('%d\t%d\n' % (c, f['hist'][c]) for c in range(2, 257))


def test_alignments_are_counted_by_their_seq_fields(X, tmp_path):
    k = 15
    want = _want(X['upper'], k, 2, tag='upper')
    got, info, _ = _count(tmp_path, 'sam.set', (), [X['sam']], k=k)
    assert got == want and info['excluded_reads'] == 0
    # -F 0x400 leaves the flagged records out of the count, not out of `reads`
    live = [r for r, fl in zip(X['upper'], X['flags']) if not fl & 0x400]
    assert 0 < len(live) < len(X['upper'])
    want_f = _want(live, k, 2, reads=len(X['upper']), tag='live')
    assert want_f != want
    got, info, _ = _count(tmp_path, 'samF.set', (), [X['sam']], k=k, exclude_flags=0x400)
    assert got == want_f and info['excluded_reads'] == len(X['upper']) - len(live)
    # a FASTQ file and an alignment file into one set; the gate reads QUAL
    assert _count(tmp_path, 'both.set', [X['fq1u']], [X['sam2']], k=k)[0] == want
    assert _count(tmp_path, 'bothQ.set', [X['fq1u']], [X['sam2']], k=k, kmer_min_qual=20)[0] == _want(X['upper'], k, 2, Q=20, tag='upper')


# ---------------------------------------------------------------- 2. unsigned order
def test_k32_keys_with_bit_63_sort_last(tmp_path):
    from kbbq import kmer
    rng = np.random.default_rng(5)
    gc = b'G' * 16 + b'C' * 16                    # its own reverse complement: the key is 10..10 01..01, bit 63 set
    rand = [bytes(LETTERS[rng.integers(0, 4, 50)]) for _ in range(6)]
    rows = [b'ACGT' + gc + b'TTGA'] * 3 + [b'A' * 40] * 2 + rand * 2 + [b'TT' + gc[:31] + b'A' + b'CCA']
    records = [(s, b'I' * len(s)) for s in rows]
    want = SM.set_bytes(records, 32, 2)
    f = SM.parse(want)
    top = int('10' * 16 + '01' * 16, 2)
    assert int(f['keys'][0]) == 0 and top in f['keys'].tolist() and int(f['keys'][-1]) >> 63 == 1
    assert (f['keys'].view(np.int64) < 0).any() and np.all(f['keys'][1:] > f['keys'][:-1])
    signed = f['keys'].view(np.int64)
    assert not np.all(signed[1:] > signed[:-1])                                  # a signed sort gives another file
    fq = _fastq(tmp_path / 'gc.fq', records)
    got, _, path = _count(tmp_path, 'gc.set', [fq], k=32)
    assert got == want
    seq, meta = M.plane(rows)
    table, hist, t, info = kmer.load_set(path, min_count=2)
    keys, counts = table.entries()
    assert np.array_equal(keys, f['keys']) and np.array_equal(counts, f['counts']) and info['loaded_kmers'] == f['n']
    table.close()
    plain, pinfo = kmer.correct_reads(seq, meta, k=32, min_count=2)
    loaded, linfo = kmer.correct_reads(seq, meta, k=None, min_count=2, kmers_from=path)
    assert np.array_equal(plain, loaded) and np.array_equal(pinfo['changed'], linfo['changed']) and int(pinfo['changed'].sum()) > 0


# ---------------------------------------------------------------- 3. sizes
def _walk(n, k, seed):
    """Two copies of one read of n + k - 1 random bases: n windows, each seen twice (asserted distinct by the caller)."""
    rng = np.random.default_rng(seed)
    s = bytes(LETTERS[rng.integers(0, 4, n + k - 1)])
    return [(s, b'I' * len(s))] * 2 + [(bytes(LETTERS[rng.integers(0, 4, 30)]), b'I' * 30)]


@pytest.mark.parametrize('n', (0, 1, 255, 256, 257))
def test_sizes_at_the_edges_of_the_sort_and_the_check(tmp_path, n):
    from kbbq import kmer
    k = 21
    records = _walk(max(n, 1), k, 100 + n)
    keep = 3 if n == 0 else 2                    # n = 0: every k-mer is below keep
    want = SM.set_bytes(records, k, keep)
    f = SM.parse(want)
    assert f['n'] == n
    fq = _fastq(tmp_path / 'w.fq', records)
    got, info, path = _count(tmp_path, 'w.set', [fq], k=k, keep=keep, slab=100)
    assert got == want and info['kmers'] == n
    for slab in (None, 100, 128, 1):
        if slab == 1 and n > 1:
            continue
        table, hist, t, linfo = kmer.load_set(path, min_count=keep, slab=slab)
        keys, counts = table.entries()
        table.close()
        assert np.array_equal(keys, f['keys']) and np.array_equal(counts, f['counts']) and t == keep
        assert np.array_equal(hist, f['hist']) and linfo['loaded_kmers'] == n and linfo['k'] == k
    # correcting against the set is correcting against the table counted here: with n = 0, against an empty table
    first = records[0][0]
    seq, meta = M.plane([s for s, _ in records] + [first[:40] + (b'T' if first[40:41] != b'T' else b'G') + first[41:]])
    plain, pinfo = kmer.correct_reads(seq, meta, k=k, min_count=keep)
    loaded, linfo = kmer.correct_reads(seq, meta, k=None, min_count=keep, kmers_from=path, slots=1024)
    assert np.array_equal(plain, loaded) and np.array_equal(pinfo['changed'], linfo['changed'])
    assert n < 255 or int(pinfo['changed'].sum()) > 0


# ---------------------------------------------------------------- 5. what the device check refuses
@pytest.fixture(scope='module')
def valid(tmp_path_factory):
    """A valid set of 257 pairs at k = 21 and one at k = 15, as bytes and fields."""
    out = {}
    for k in (21, 15):
        data = SM.set_bytes(_walk(257, k, 357), k, 2)
        f = SM.parse(data)
        assert f['n'] == 257
        out[k] = (data, f)
    out['dir'] = tmp_path_factory.mktemp('kmer_set_bad')
    return out


def _noncanonical_above(f, k):
    """A key that is above its reverse complement and above the set's last but one key: it can take the last key's place."""
    for key in f['keys'].tolist():
        rc = M.revcomp(int(key), k)
        if rc > int(f['keys'][-2]) and rc > int(key):
            return rc
    raise AssertionError('no candidate')


TAMPERINGS = ('swapped', 'duplicate', 'duplicate-across-slabs', 'non-canonical', 'out-of-range', 'low-count', 'checksum')


@pytest.mark.parametrize('how', TAMPERINGS)
def test_the_device_check_names_the_pair(valid, X, tmp_path, how):
    from kbbq import kmer
    k = 15 if how == 'out-of-range' else 21
    data, f = valid[k]
    keys, counts = f['keys'].copy(), f['counts'].copy()
    slab = None
    if how == 'swapped':
        keys[[40, 41]] = keys[[41, 40]]
    elif how == 'duplicate':
        keys[10] = keys[9]
    elif how == 'duplicate-across-slabs':
        keys[100], slab = keys[99], 100          # pair 100 is the first of the second slab: prev_key hands keys[99] over
    elif how == 'non-canonical':
        keys[-1] = _noncanonical_above(f, k)
    elif how == 'out-of-range':
        keys[-1] = 4 ** 15 + 5
    elif how == 'low-count':
        counts[7] = 1
    bad = SM.retouch(data, keys, counts)
    if how == 'checksum':
        bad = data[:48] + (f['key_sum'] + 1).to_bytes(8, 'little') + data[56:]
    g = SM.parse(bad)
    found = SM.check_pairs(g['keys'], g['counts'], k, 2, g['key_sum'], g['count_sum'])
    expected = dict(swapped=(41, SM.ORDER), duplicate=(10, SM.ORDER), **{'duplicate-across-slabs': (100, SM.ORDER)},
                    **{'non-canonical': (256, SM.CANONICAL), 'out-of-range': (256, SM.RANGE), 'low-count': (7, SM.COUNT)}).get(how, 'checksum')
    assert found == expected
    path = str(tmp_path / 'bad.set')
    with open(path, 'wb') as fh:
        fh.write(bad)
    message = 'checksum' if found == 'checksum' else r'pair %d: %s' % (found[0], re.escape(kmer.PAIR_REASONS[found[1]]))
    for s in (slab, None) if slab else (None, 64):
        with pytest.raises(ValueError, match=r'k-mer set .*bad\.set: ' + message):
            kmer.load_set(path, min_count=2, slab=s)
    # no corrected byte is written, and the context goes on: a valid load and a correction follow
    out = str(tmp_path / 'never.fq')
    with pytest.raises(ValueError, match=message):
        kmer.correct_fastq(X['fq'], out, k=None, min_count=2, kmers_from=path)
    assert not os.path.exists(out)
    good = str(tmp_path / 'good.set')
    with open(good, 'wb') as fh:
        fh.write(data)
    table, _, _, info = kmer.load_set(good, min_count=2, slab=slab)
    got = table.entries()
    table.close()
    assert np.array_equal(got[0], f['keys']) and np.array_equal(got[1], f['counts']) and info['loaded_kmers'] == 257


def test_the_check_kernel_on_unaligned_slabs_and_its_sums(valid):
    """kmer.check_pairs itself: slabs that start at odd pairs (the plain loads) give the model's answer and sums that add up."""
    import torch
    from kbbq import kmer
    data, f = valid[21]
    keys, counts = f['keys'].copy(), f['counts'].copy()
    counts[200] = 1
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    sums = np.zeros(2, dtype=np.uint64)
    found = []
    for lo, hi in ((0, 1), (1, 4), (4, 131), (131, 257)):
        _, bad = kmer.check_pairs(d_keys[lo:hi], d_counts[lo:hi], 21, 2, first=lo, prev=int(keys[lo - 1]) if lo else None, sums=sums)
        found.append(bad)
    assert found[:3] == [None, None, None] and found[3] == (200, kmer.PAIR_REASONS[SM.COUNT])
    assert int(sums[0]) == f['key_sum'] and int(sums[1]) == f['count_sum'] - 1
    # a slab that repeats the key before it is told so only when that key is handed over
    assert kmer.check_pairs(d_keys[5:9], d_counts[5:9], 21, 2, first=5, prev=int(keys[5]))[1] == (5, kmer.PAIR_REASONS[SM.ORDER])
    assert kmer.check_pairs(d_keys[5:9], d_counts[5:9], 21, 2, first=5)[1] is None
    # the sort: a shuffled copy comes back as the file's order, keys with their counts
    perm = np.random.default_rng(1).permutation(257)
    pieces = [(torch.from_numpy(f['keys'][perm[a:b]].view(np.int64).copy()).cuda(), torch.from_numpy(f['counts'][perm[a:b]].view(np.int32).copy()).cuda())
              for a, b in ((0, 100), (100, 100), (100, 257))]
    sk, sc = kmer.sort_pairs(pieces, 21)
    assert pieces == [] and np.array_equal(sk.cpu().numpy().view(np.uint64), f['keys']) and np.array_equal(sc.cpu().numpy().view(np.uint32), f['counts'])


# ---------------------------------------------------------------- 4. the five commands
@pytest.fixture
def kbbq(monkeypatch, capfdbinary):
    """The command line in this process: main.main(argv) -> (stdout bytes, its `kbbq ...:` lines of stderr)."""
    from kbbq import main
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                      # this process has torch tensors already
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED'):
        monkeypatch.delenv(var, raising=False)

    def run(*argv):
        capfdbinary.readouterr()
        main.main([str(a) for a in argv])
        sys.stdout.flush()
        sys.stderr.flush()
        out, err = capfdbinary.readouterr()
        return out, [ln for ln in err.decode().split('\n') if ln.startswith('kbbq ')]
    return run


def _with_field(line, n):
    return line + ' kmers_from=1 loaded_kmers=%d' % n


def test_correct_and_recalibrate_c_from_a_set(X, kbbq, tmp_path):
    k = 15
    f = SM.parse(_want(X['records'], k, 2))
    t = M.threshold(f['hist'])                   # the valley the commands find themselves, checked on the model first
    assert t >= 2 and int((f['counts'] >= t).sum()) > 0
    s = str(tmp_path / 'x.set')
    out, said = kbbq('count', '-f', X['fq1'], X['fq2'], '-o', s, '-k', k, '--prefilter')
    assert out == b'' and open(s, 'rb').read() == _want(X['records'], k, 2)
    assert re.fullmatch(r'kbbq count: k=15 keep=2 inputs=2 reads=%d windows=%d kmers=%d valley=%d prefilter=1 admitted=\d+ slots=\d+'
                        % (len(X['records']), int(np.maximum(X['meta'].astype(np.int64) - k + 1, 0).sum()), f['n'], t), said[0]), said
    for opts in ((), ('--fix-n', '--passes', '3'), ('--min-count', '4', '--passes', '2')):
        want, line = kbbq('correct', '-f', X['fq'], '-k', k, *opts)
        got, said = kbbq('correct', '-f', X['fq'], '--kmers-from', s, *opts)
        assert got == want and want.count(b'\n') == 4 * len(X['records']) and said == [_with_field(line[0], f['n'])]
        assert (' min_count=%d ' % (4 if '--min-count' in opts else t)) in line[0]
    a, b = tmp_path / 'a.fq', tmp_path / 'b.fq'
    kbbq('correct', '-f', X['fq'], '-k', k, '-o', a)
    assert kbbq('correct', '-f', X['fq'], '--kmers-from', s, '-k', k, '-o', b)[0] == b'' and a.read_bytes() == b.read_bytes()
    assert a.read_bytes() == kbbq('correct', '-f', X['fq'], '-k', k)[0]
    # recalibrate -c (reads of 40 bases and more, upper case): stdout, the report and the line
    sl = str(tmp_path / 'long.set')
    kbbq('count', '-f', X['fqlong'], '-o', sl, '-k', k, '--partitions', '2')
    nl = SM.parse(open(sl, 'rb').read())['n']
    assert open(sl, 'rb').read() == _want(X['long'], k, 2, tag='long')
    for opts in ((), ('--skip-unresolved', '--fix-n')):
        g1, g2 = tmp_path / ('one%d.grp' % len(opts)), tmp_path / ('two%d.grp' % len(opts))
        want, line = kbbq('recalibrate', '-c', X['fqlong'], '-k', k, '-g', g1, *opts)
        got, said = kbbq('recalibrate', '-c', X['fqlong'], '--kmers-from', sl, '-g', g2, *opts)
        assert got == want and len(want) > 1000 and g1.read_bytes() == g2.read_bytes() and said == [_with_field(line[0], nl)]
    # a --min-count below the set's keep, and a -k that is not the set's
    with pytest.raises(ValueError, match='min_count = 1 is below keep = 2'):
        kbbq('correct', '-f', X['fq'], '--kmers-from', s, '--min-count', '1')
    with pytest.raises(ValueError, match='k = 21 was asked for, but the k-mer set .* was counted with k = 15'):
        kbbq('correct', '-f', X['fq'], '--kmers-from', s, '-k', '21')


@pytest.fixture(scope='module')
def aligned(tmp_path_factory):
    """kmer_bqsr_model.FIXTURE (600 records of 60 bases, truth set included), and the same with every fifth record cut to 45 bases
    and every seventh flagged as a duplicate."""
    import kmer_bqsr_model as B
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('kmer_set_aligned')
    paths = OQ.synth_bqsr_set(str(d), **B.FIXTURE)
    lines = open(paths['sam']).read().split('\n')
    out, i = [], 0
    for ln in lines:
        if ln and not ln.startswith('@'):
            fld = ln.split('\t')
            if i % 5 == 2:
                fld[5], fld[9], fld[10] = '45M', fld[9][:45], fld[10][:45]
                fld = [x if not x.startswith('OQ:Z:') else x[:5 + 45] for x in fld]
            if i % 7 == 3:
                fld[1] = str(int(fld[1]) | 0x400)
            ln = '\t'.join(fld)
            i += 1
        out.append(ln)
    mixed = d / 'mixed.sam'
    mixed.write_text('\n'.join(out))
    return dict(paths=paths, mixed=str(mixed), dir=d)


def test_bqsr_recalibrate_b_and_benchmark_from_a_set(aligned, kbbq, tmp_path):
    p = aligned['paths']
    s, sm = str(tmp_path / 'aln.set'), str(tmp_path / 'mixed.set')
    kbbq('count', '-b', p['sam'], '-o', s, '-k', '15')
    n = SM.parse(open(s, 'rb').read())['n']
    kbbq('count', '-b', aligned['mixed'], '-F', '0x400', '-o', sm, '-k', '15', '--partitions', '2')
    nm = SM.parse(open(sm, 'rb').read())['n']
    assert 0 < nm != n
    # bqsr --kmers
    for sam, the_set, loaded, opts in ((p['sam'], s, n, ('--skip-unresolved',)),
                                       (aligned['mixed'], sm, nm, ('--skip-unresolved', '--mixed-lengths', '-F', '0x400', '--passes', '2',
                                                                   '--min-count', '3'))):
        g1, g2 = tmp_path / 'one.grp', tmp_path / 'two.grp'
        _, line = kbbq('bqsr', '-b', sam, '--kmers', '-k', '15', '-g', g1, *opts)
        _, said = kbbq('bqsr', '-b', sam, '--kmers', '--kmers-from', the_set, '-g', g2, *opts)
        assert g1.read_bytes() == g2.read_bytes() and len(g1.read_bytes()) > 1000 and said == [_with_field(line[0], loaded)]
    # recalibrate -b --kmers: stdout, -o, the report
    g1, g2, o2 = tmp_path / 'r1.grp', tmp_path / 'r2.grp', tmp_path / 'r2.sam'
    want, line = kbbq('recalibrate', '-b', p['sam'], '--kmers', '-k', '15', '-g', g1)
    got, said = kbbq('recalibrate', '-b', p['sam'], '--kmers', '--kmers-from', s, '-g', g2, '-o', o2)
    assert got == b'' and o2.read_bytes() == want and want.count(b'\n') > 600 and g1.read_bytes() == g2.read_bytes()
    assert said == [_with_field(line[0], n)]
    # benchmark --kmers
    base = ('benchmark', '-b', p['sam'], '-r', p['fa'], '-v', p['vcf'], '-l', 'lbl', '--kmers')
    want, line = kbbq(*base, '-k', '15', '--passes', '2')
    got, said = kbbq(*base, '--kmers-from', s, '--passes', '2')
    assert got == want and want.count(b'\n') > 5 and said == [_with_field(line[0], n)]


def test_count_the_fastq_decide_the_alignments(aligned, tmp_path):
    """The raw reads (every second record of the alignments, reverse-strand ones turned back) counted as FASTQ; the alignments'
    errors decided by that set are the model's with the FASTQ's k-mers in the place of the alignments' own."""
    import kmer_bqsr_model as B
    from kbbq import aln, kmerset
    from kbbq.gatk import bqsr
    k, t = 15, 3
    reads, rgs, _ = B.load(aligned['paths']['sam'])
    comp = bytes.maketrans(b'ACGT', b'TGCA')
    raw = []
    for r in reads[::2]:
        s = r.query_sequence.encode()
        raw.append((s.translate(comp)[::-1] if r.is_reverse else s, b'I' * len(s)))
    fq = _fastq(tmp_path / 'raw.fq', raw)
    s = str(tmp_path / 'raw.set')
    kmerset.count([fq], (), s, k=k)
    assert open(s, 'rb').read() == SM.set_bytes(raw, k, 2)
    keys, counts = SM.count(raw, k)
    seq, meta = B.planes(reads)
    plain, M.count, M.np = M.count, (lambda *_: (keys, counts)), G._PlainIndices()
    try:
        out = M.correct(seq, meta, k, t)[0]
    finally:
        M.count, M.np = plain, np
    own = B.flags(reads, k, t)[0]
    assert (out != seq).any() and not np.array_equal(out != seq, own)             # another set, other decisions
    want, _ = B.vectors(reads, rgs, k, t, flagged=(out != seq, t))
    info = {}
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(aligned['paths']['sam']), k=None, min_count=t, kmers_from=s, info=info)
    for name, g, w in zip(B.VEC, got, want):
        assert np.array_equal(g, w), name
    assert info['k'] == k and info['min_count'] == t and info['loaded_kmers'] == SM.parse(open(s, 'rb').read())['n']
