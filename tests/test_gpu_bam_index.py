"""--bam-index on the MI355X: the index kernels (kbbq_bam_index_dev, csrc/kbbq_bam_index.h) against their host twin on the slabs of
tests/bam_index_cases.py -- runs, linear array, n_no_coor -- and the two commands end to end: the index written beside the BAM is
tests/bam_index_model.py's index of that BAM, the BAM is the one written without the option, whatever the slabs are."""
import ctypes
import sys

import numpy as np
import pytest

import bam_index_cases as K
import bam_index_model as M
import bam_out_cases as C

pytestmark = pytest.mark.gpu

ONES = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------- the kernels against their host twin
@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp('bam_index_gpu')
    rng = np.random.default_rng(41)
    out = {}
    for name, lines, header in (('edges', K.edges(rng), K.HEADER), ('many', K.many(rng), K.HEADER), ('block_end', K.block_end(rng)[0], K.HEADER),
                                ('long_cigar', K.long_cigar(rng), K.HEADER), ('big', K.big(rng), K.BIG)):
        sub = d / name
        sub.mkdir()
        out[name] = K.parsed(sub, lines, header)
    return out


def _windows(case):
    from kbbq import _bamindex
    lengths = [ln for _, ln, _ in _bamindex.references(case['bam'].header)]
    lin_off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    lin_off[1:] = np.cumsum(np.array(_bamindex.window_counts(lengths), dtype=np.uint64))
    return lin_off, _bamindex.depth_for(max(lengths))


def _host(desc, skel, base, depth, lin_off, linear):
    from kbbq import _native as N
    n = len(desc)
    runs = np.zeros(n * N.BAM_RUN_BYTES, dtype=np.uint8)
    count, bad = ctypes.c_int64(-5), ctypes.c_int64(-5)
    rc = N.load().kbbq_bam_index(N.ptr(skel), skel.nbytes, N.ptr(desc), n, base, depth, N.ptr(lin_off), len(lin_off) - 1, N.ptr(linear),
                                 N.ptr(runs), n, ctypes.byref(count), ctypes.byref(bad))
    return rc, runs[:count.value * N.BAM_RUN_BYTES].tobytes(), int(bad.value)


def _device(desc, skel, base, depth, lin_off, d_linear):
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    ctx = dev.context()
    n = len(desc)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()      # noqa: E731
    d_skel, d_desc, d_lin_off = up(skel if skel.size else np.zeros(1, np.uint8)), up(desc), up(lin_off)
    runs = np.zeros(n * N.BAM_RUN_BYTES, dtype=np.uint8)
    count, bad = ctypes.c_int64(-5), ctypes.c_int64(-5)
    rc = N.load().kbbq_bam_index_dev(ctx.handle, N.ptr(d_skel), skel.nbytes, N.ptr(d_desc), n, base, depth, N.ptr(d_lin_off),
                                     len(lin_off) - 1, N.ptr(d_linear), N.ptr(runs), n, ctypes.byref(count), ctypes.byref(bad))
    return rc, runs[:count.value * N.BAM_RUN_BYTES].tobytes(), int(bad.value)


SLABS = [('edges', 1000), ('edges', 1), ('edges', 5), ('many', 2000), ('many', 257), ('many', 64), ('block_end', 1000), ('long_cigar', 2),
         ('big', 1000), ('big', 3)]


@pytest.mark.parametrize('name,rows', SLABS, ids=['%s-%d' % s for s in SLABS])
def test_the_kernels_against_their_host_twin(cases, name, rows):
    import torch
    from kbbq import _bamindex
    case = cases[name]
    bam, n = case['bam'], len(case['bam'])
    lin_off, depth = _windows(case)
    assert depth == (6 if name == 'big' else 5)
    total = int(lin_off[-1])
    linear = np.full(total, ONES, dtype=np.uint64)
    d_linear = torch.from_numpy(linear.view(np.int64).copy()).cuda()
    base, no_coor, all_runs = 1234567, [0, 0], 0
    for first in range(0, n, rows):
        m = min(rows, n - first)
        desc, skel, size = C.layout(bam, True, case['keep'], first, m)
        rc_h, runs_h, bad_h = _host(desc, skel, base, depth, lin_off, linear)
        rc_d, runs_d, bad_d = _device(desc, skel, base, depth, lin_off, d_linear)
        assert rc_h == rc_d == 0 and bad_h == bad_d == -1
        assert runs_d == runs_h and len(runs_h) >= 32
        for k, runs in enumerate((runs_h, runs_d)):
            r = np.frombuffer(runs, dtype=_bamindex.RUN)
            assert int(r['n_mapped'].sum() + r['n_unmapped'].sum()) == m and r['beg'][0] == base and r['end'][-1] == base + size
            assert np.all(r['beg'][1:] == r['end'][:-1])
            no_coor[k] += int((r['n_mapped'] + r['n_unmapped'])[r['ref'] < 0].sum())
        all_runs += len(runs_h) // 32
        base += size
    got = d_linear.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, linear) and (linear != ONES).any()
    want_no_coor = sum(1 for ln in case['text'].split('\n') if ln and ln[0] != '@' and ln.split('\t')[2] == '*')
    assert no_coor == [want_no_coor, want_no_coor]
    assert name != 'many' or 50 < all_runs < n // 10                 # runs, not records: a few dozen for 1500 records


def test_more_than_one_workgroup_of_runs_and_of_one_run():
    """Synthetic heads alone (no file), 1000 records: every record a bin of its own (four workgroups of heads), three records a
    bin, all in one bin."""
    import struct
    import torch
    n, windows = 1000, 700
    lin_off = np.array([0, windows], dtype=np.uint64)
    for step, want_runs in ((16384, n), (5462, 334), (0, 1)):
        desc = np.zeros((n, 6), dtype=np.uint32)
        skel = bytearray()
        at = 0
        for r in range(n):
            size = 60 + r % 7
            # block_size, refID 0, pos, l_read_name 4, mapq, bin, n_cigar_op 1, flag, l_seq, next_refID, next_pos, tlen, QNAME, 10M
            skel += struct.pack('<iiiBBHHHiiii4sI', size, 0, r * step, 4, 0, 0, 1, 4 if r % 5 == 0 else 0, 0, -1, -1, 0, b'abc', 10 << 4)
            desc[r] = (44 * r, 44, 0, 0, at, 0)
            at += 4 + size
        skel = np.frombuffer(bytes(skel), dtype=np.uint8)
        linear = np.full(windows, ONES, dtype=np.uint64)
        d_linear = torch.from_numpy(linear.view(np.int64).copy()).cuda()
        rc_h, runs_h, bad_h = _host(desc, skel, 99, 5, lin_off, linear)
        rc_d, runs_d, bad_d = _device(desc, skel, 99, 5, lin_off, d_linear)
        assert rc_h == rc_d == 0 and bad_h == bad_d == -1 and runs_h == runs_d
        assert len(runs_h) == 32 * want_runs
        assert np.array_equal(d_linear.cpu().numpy().view(np.uint64), linear)
        assert (linear != ONES).sum() == {16384: windows, 5462: 334, 0: 1}[step]
        if step == 16384:                                            # windows past the reference's last are clamped to it: the lowest start
            assert linear[windows - 1] == 99 + int(desc[windows - 1, 4])


def test_a_record_that_does_not_fit_touches_nothing(cases):
    import torch
    case = cases['many']
    lin_off, depth = _windows(case)
    desc, skel, size = C.layout(case['bam'], False, case['keep'], 0, 600)
    for broken, row in (('skel', 300), ('head', 77), ('ref', 0)):
        d = desc.copy()
        args = dict(skel=skel, lin_off=lin_off)
        if broken == 'skel':
            args['skel'] = skel[:int(desc[300, 0]) + 20]             # the skeleton ends inside the head of row 300
        elif broken == 'head':
            d[77, 1] = 36
        else:
            args['lin_off'] = lin_off[:1].copy()                     # no references at all: every refID is beyond them
        linear = np.full(max(int(args['lin_off'][-1]), 1), ONES, dtype=np.uint64)
        d_linear = torch.from_numpy(linear.view(np.int64).copy()).cuda()
        rc_h, _, bad_h = _host(d, args['skel'], 0, depth, args['lin_off'], linear)
        rc_d, runs_d, bad_d = _device(d, args['skel'], 0, depth, args['lin_off'], d_linear)
        assert rc_h == rc_d == -4 and bad_h == bad_d == row and runs_d == b''
        if broken != 'skel':                                         # (rows below the bad one may have filled their windows on the device)
            assert np.all(linear == ONES)
        got = d_linear.cpu().numpy().view(np.uint64)
        if broken == 'ref':
            assert np.all(got == ONES)


# ---------------------------------------------------------------- end to end
@pytest.fixture
def kbbq(monkeypatch, capfdbinary):
    """The command line in this process: main.main(argv) -> (stdout bytes, stderr text)."""
    from kbbq import main
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)

    def run(*argv):
        capfdbinary.readouterr()
        main.main([str(a) for a in argv])
        sys.stdout.flush()
        sys.stderr.flush()
        out, err = capfdbinary.readouterr()
        return out, err.decode()
    return run


def _report(path, rng):
    from kbbq.gatk import bqsr
    R, Q, S2 = 3, 43, 300
    q_total = rng.integers(0, 5000, (R, Q))
    q_errs = (q_total * rng.uniform(0, 0.05, (R, Q))).astype(np.int64)
    pos_total = rng.integers(0, 200, (R, Q, S2))
    pos_errs = (pos_total * rng.uniform(0, 0.1, (R, Q, S2))).astype(np.int64)
    dn_total = rng.integers(0, 800, (R, Q, 16))
    dn_errs = (dn_total * rng.uniform(0, 0.1, (R, Q, 16))).astype(np.int64)
    report = bqsr.vectors_to_report(np.zeros(R), q_errs.sum(1), q_total.sum(1), q_errs, q_total, pos_errs, pos_total, dn_errs, dn_total,
                                    ['pu0', 'pu1', 'pu2'])
    path.write_text(str(report))
    return str(path)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """`many` (BAI territory) and `big` with `many`'s records behind it on the long reference (CSI), as SAM files; a report."""
    d = tmp_path_factory.mktemp('bam_index_e2e')
    rng = np.random.default_rng(8)
    (d / 'many.sam').write_text(C.sam_text(K.many(rng), K.HEADER))
    moved = [ln.replace('\tchr1\t', '\twheat3B\t').replace('\tchr2\t', '\twheat3B\t') for ln in K.many(rng, 600) if '\tchrM\t' not in ln]
    (d / 'big.sam').write_text(C.sam_text(K._sorted(K.big(rng) + moved, K.BIG), K.BIG))
    return dict(dir=d, many=str(d / 'many.sam'), big=str(d / 'big.sam'), report=_report(d / 'model.grp', rng))


def _index_of(path, fmt):
    data = open('%s.%s' % (path, fmt), 'rb').read()
    if fmt == 'csi':
        assert M.crc_ok(data)
        return M.inflate(data), len(data)
    return data, len(data)


@pytest.mark.parametrize('source,kind,fmt', [('many', (), 'bai'), ('many', ('bai',), 'bai'), ('many', ('csi',), 'csi'), ('big', (), 'csi'),
                                             ('big', ('auto',), 'csi'), ('big', ('csi',), 'csi')],
                         ids=['many-bare', 'many-bai', 'many-csi', 'big-bare', 'big-auto', 'big-csi'])
def test_applybqsr_writes_the_index_the_model_gives(files, kbbq, tmp_path, source, kind, fmt):
    import os
    from kbbq.gatk import applybqsr
    plain, out = tmp_path / 'plain.bam', tmp_path / 'out.bam'
    said_plain = kbbq('applybqsr', '-b', files[source], '-g', files['report'], '-s', '--bam-out', '-o', plain)
    (tmp_path / ('out.bam.' + fmt)).write_bytes(b'stale' * 100000)   # an existing index is overwritten
    said = kbbq('applybqsr', '-b', files[source], '-g', files['report'], '-s', '--bam-out', '--bam-index', *kind, '-o', out)
    assert said == said_plain and said[0] == b''                     # stderr is what it was
    data = out.read_bytes()
    assert data == plain.read_bytes()                                # ... and so is the BAM
    assert sorted(os.listdir(tmp_path)) == ['out.bam', 'out.bam.' + fmt, 'plain.bam']
    got, size = _index_of(out, fmt)
    want, want_fmt, depth = M.build(data, kind[0] if kind else 'auto')
    assert want_fmt == fmt and depth == (6 if source == 'big' else 5)
    assert got == want
    counters = dict(applybqsr.LAST_RUN['bam_out'])
    assert counters['index_bytes'] == size and counters['index_runs'] > 10 and counters['file_bytes'] == len(data)
    assert counters['index_d2h_bytes'] > 32 * counters['index_runs']     # the runs, and the linear array once
    index = M.parse(want)
    assert index['n_no_coor'] == (5 if source == 'many' else 6) and any(entry['meta'] for entry in index['refs'])


def test_bai_is_refused_for_the_long_reference_before_any_file(files, kbbq, tmp_path):
    out = tmp_path / 'never.bam'
    with pytest.raises(ValueError, match='@SQ SN:wheat3B LN:536870913'):
        kbbq('applybqsr', '-b', files['big'], '-g', files['report'], '--bam-out', '--bam-index', 'bai', '-o', out)
    assert list(tmp_path.iterdir()) == []


def test_the_index_does_not_depend_on_the_slabs(files, kbbq, tmp_path, monkeypatch):
    from kbbq.gatk import applybqsr
    one = tmp_path / 'one.bam'
    kbbq('applybqsr', '-b', files['many'], '-g', files['report'], '--bam-out', '--bam-index', '-o', one)
    runs = applybqsr.LAST_RUN['bam_out']['index_runs']
    want = (one.read_bytes(), _index_of(one, 'bai')[0])
    monkeypatch.setattr(applybqsr, '_ROWS', 64)                      # two dozen slabs: runs and records straddle the cuts
    again = tmp_path / 'again.bam'
    kbbq('applybqsr', '-b', files['many'], '-g', files['report'], '--bam-out', '--bam-index', '-o', again)
    assert (again.read_bytes(), _index_of(again, 'bai')[0]) == want
    assert applybqsr.LAST_RUN['bam_out']['index_runs'] == runs       # a run cut by a slab is joined again
    monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '1')
    kbbq('applybqsr', '-b', files['many'], '-g', files['report'], '--bam-out', '--bam-index', '-o', again)
    assert (again.read_bytes(), _index_of(again, 'bai')[0]) == want
    kbbq('applybqsr', '-b', files['big'], '-g', files['report'], '--bam-out', '--bam-index', '-o', again)
    monkeypatch.delenv('KBBQ_BGZF_SLAB_BLOCKS')
    monkeypatch.setattr(applybqsr, '_ROWS', 1 << 20)
    kbbq('applybqsr', '-b', files['big'], '-g', files['report'], '--bam-out', '--bam-index', '-o', one)
    assert (again.read_bytes(), _index_of(again, 'csi')[0]) == (one.read_bytes(), _index_of(one, 'csi')[0])


def test_only_runs_cross_the_bus(files, kbbq, tmp_path):
    """All records in one bin: what comes back for the index does not grow with the records -- one run a slab."""
    from kbbq.gatk import applybqsr
    rng = np.random.default_rng(12)
    back = {}
    for n in (1000, 4000):
        lines = [K.record(rng, 'r%d' % k, 'chr1', 100 + 3 * k, L=40, tags=('RG:Z:rg%d' % (k % 3),)) for k in range(n)]
        path = tmp_path / ('%d.sam' % n)
        path.write_text(C.sam_text(lines, K.HEADER))
        out = tmp_path / ('%d.bam' % n)
        kbbq('applybqsr', '-b', path, '-g', files['report'], '--bam-out', '--bam-index', '-o', out)
        counters = applybqsr.LAST_RUN['bam_out']
        assert counters['index_runs'] == 1
        assert _index_of(out, 'bai')[0] == M.build(out.read_bytes(), 'bai')[0]
        back[n] = counters['index_d2h_bytes']
    assert back[1000] == back[4000] > 0


def test_recalibrate_kmers_writes_the_index_too(kbbq, tmp_path):
    """`recalibrate -b --kmers --bam-out --bam-index` over test_gpu_recalibrate_bam's input, sorted by coordinate."""
    import kmer_bqsr_model as B
    import oracle_bqsr as OQ
    from kbbq import recalibrate
    text = open(OQ.synth_bqsr_set(str(tmp_path), **B.FIXTURE)['sam']).read()
    header = [ln for ln in text.split('\n') if ln.startswith('@')]
    lines = K._sorted([ln for ln in text.split('\n') if ln and not ln.startswith('@')], header)
    sam = tmp_path / 'sorted.sam'
    sam.write_text(C.sam_text(lines, header))
    plain, out = tmp_path / 'plain.bam', tmp_path / 'out.bam'
    k = ('-k', '15')
    said_plain = kbbq('recalibrate', '-b', sam, '--kmers', *k, '-s', '--bam-out', '-g', tmp_path / 'plain.grp', '-o', plain)
    said = kbbq('recalibrate', '-b', sam, '--kmers', *k, '-s', '--bam-out', '--bam-index', '-g', tmp_path / 'out.grp', '-o', out)
    assert said == said_plain and said[1].startswith('kbbq recalibrate: k=15')
    assert out.read_bytes() == plain.read_bytes() and (tmp_path / 'out.grp').read_bytes() == (tmp_path / 'plain.grp').read_bytes()
    assert _index_of(out, 'bai')[0] == M.build(out.read_bytes(), 'bai')[0]
    assert recalibrate.LAST_RUN['aligned']['alignments'] == len(lines)
    # unsorted, the same command refuses before the report or the file exists
    never = tmp_path / 'never.bam'
    with pytest.raises(ValueError, match='out of coordinate order') as err:
        kbbq('recalibrate', '-b', OQ.synth_bqsr_set(str(tmp_path), **B.FIXTURE)['sam'], '--kmers', *k, '--bam-out', '--bam-index', '-g',
             tmp_path / 'never.grp', '-o', never)
    assert err.value.read_index > 0 and not never.exists() and not (tmp_path / 'never.grp').exists()


def test_the_command_as_a_process_of_its_own(tmp_path):
    """`recalibrate -b --kmers` on one GPU imports no torch: the linear array and the index's buffers then come from the library's
    own allocator (kbbq/_hipmem.py).  The same BAM, and its model's index."""
    import os
    import subprocess
    import kmer_bqsr_model as B
    import oracle_bqsr as OQ
    text = open(OQ.synth_bqsr_set(str(tmp_path), **B.FIXTURE)['sam']).read()
    header = [ln for ln in text.split('\n') if ln.startswith('@')]
    sam = tmp_path / 'sorted.sam'
    sam.write_text(C.sam_text(K._sorted([ln for ln in text.split('\n') if ln and not ln.startswith('@')], header), header))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, 'kbbq-py_amd'))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS'):
        env.pop(var, None)
    base = [sys.executable, '-m', 'kbbq.main', 'recalibrate', '-b', str(sam), '--kmers', '-k', '15', '-s', '--bam-out']
    plain = subprocess.run(base + ['-o', str(tmp_path / 'plain.bam')], env=env, capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()
    out = tmp_path / 'p.bam'
    made = subprocess.run(base + ['--bam-index', 'csi', '-o', str(out)], env=env, capture_output=True, timeout=120)
    assert made.returncode == 0 and made.stdout == b'' and made.stderr == plain.stderr, made.stderr.decode()
    assert out.read_bytes() == (tmp_path / 'plain.bam').read_bytes()
    assert _index_of(out, 'csi')[0] == M.build(out.read_bytes(), 'csi')[0]
