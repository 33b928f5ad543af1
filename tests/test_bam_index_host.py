"""--bam-index without a GPU: the executable model's known answers, kbbq/_bamout.py's BamWriter with index= over the host twin
(kbbq_bam_index) and a zlib stand-in for the deflate call against tests/bam_index_model.py applied to the written BAM, the query
property of every record, and the refusals -- each before the output file exists."""
import ctypes
import os

import numpy as np
import pytest

import bam_index_cases as K
import bam_index_model as M
import bam_out_cases as C
from test_bgzf_host import BLOCK, EOF, zlib_blocks


# ---------------------------------------------------------------- the model
def test_known_answers_of_the_model():
    assert M.reg2bin(0, 1) == 4681
    assert M.reg2bin(16384, 16385) == 4682
    assert M.reg2bin(16383, 16385) == 585
    assert M.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    assert M.pseudo_bin('bai', 5) == 37450 == M.pseudo_bin('csi', 5)
    assert M.depth_for((1 << 29) + 1) == 6 and M.depth_for(1 << 29) == 5 and M.depth_for(1) == 5
    assert M.pseudo_bin('csi', 6) == ((1 << 21) - 1) // 7 + 1
    # depth 6: the finest bins begin at (8^6 - 1) / 7, and 2^29 is the first base of the second level-1 bin
    assert M.reg2bin(0, 1, 14, 6) == 37449 and M.reg2bin(1 << 29, (1 << 29) + 1, 14, 6) == 37449 + (1 << 15)
    assert M.reg2bin((1 << 29) - 1, (1 << 29) + 1, 14, 6) == 0
    assert 4681 in M.reg2bins(0, 1) and M.reg2bins(0, 1) == [0, 1, 9, 73, 585, 4681]
    from kbbq import _bamindex
    assert _bamindex.depth_for((1 << 29) + 1) == 6 and _bamindex.window_counts([16569, 0, 16384]) == [3, 2, 2]


# ---------------------------------------------------------------- the host twin against the model
@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp('bam_index')
    rng = np.random.default_rng(41)
    out = {}
    for name, lines, header in (('edges', K.edges(rng), K.HEADER), ('many', K.many(rng), K.HEADER), ('block_end', K.block_end(rng)[0], K.HEADER),
                                ('long_cigar', K.long_cigar(rng), K.HEADER), ('big', K.big(rng), K.BIG), ('header_only', [], K.HEADER),
                                ('one', K.edges(rng)[:1], K.HEADER)):
        sub = d / name
        sub.mkdir()
        out[name] = K.parsed(sub, lines, header)
    return out


def _inflated(writer):
    data = writer.index_data
    if writer.index_format == 'csi':
        assert M.crc_ok(data)
        return M.inflate(data)
    return data


SHAPES = [('edges', 1000, 'auto'), ('edges', 1, 'bai'), ('edges', 5, 'csi'), ('many', 2000, 'auto'), ('many', 64, 'bai'), ('many', 7, 'csi'),
          ('many', 499, 'auto'), ('block_end', 1000, 'bai'), ('block_end', 50, 'csi'), ('long_cigar', 3, 'auto'), ('long_cigar', 1, 'csi'),
          ('big', 100, 'auto'), ('big', 2, 'csi'), ('header_only', 10, 'bai'), ('header_only', 10, 'csi'), ('one', 1, 'auto')]


@pytest.mark.parametrize('name,rows,kind', SHAPES, ids=['%s-%d-%s' % s for s in SHAPES])
def test_the_host_twin_against_the_model(cases, monkeypatch, name, rows, kind):
    case = cases[name]
    if rows in (7, 50):
        monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '1')
    data, w = K.written(case, rows, kind, zlib_blocks)
    plain, _ = K.written(case, rows, None, zlib_blocks)
    assert data == plain and data.endswith(EOF)                      # the BAM itself is what it was
    want, fmt, depth = M.build(data, kind)
    assert w.index_format == fmt == ('csi' if kind == 'csi' or name == 'big' else 'bai')
    assert depth == (6 if name == 'big' else 5)
    assert _inflated(w) == want
    assert w.index_bytes == len(w.index_data) and w.index_d2h_bytes == 0 and w.index_runs >= (len(case['bam']) > 0)
    index = M.parse(want)
    assert index['n_no_coor'] == sum(1 for ln in case['text'].split('\n') if ln and ln[0] != '@' and ln.split('\t')[2] == '*')
    assert len(index['refs']) == sum(1 for ln in case['text'].split('\n') if ln.startswith('@SQ'))


def test_the_shapes_the_cases_are_there_for(cases):
    """What each case promises is in it (by the model's reading of the written file)."""
    data, _ = K.written(cases['many'], 64, 'bai', zlib_blocks)
    bam = M.Bam(data)
    assert len(bam.members) >= 4 and any(r['start'] // BLOCK != (r['stop'] - 1) // BLOCK for r in bam.records)       # over a block cut
    firsts = [bam.records[k] for k in range(64, len(bam.records), 64)]
    assert any(r['start'] % BLOCK for r in firsts)                                                                    # carried below a block
    same = [M.reg2bin(a['beg'], a['end']) == M.reg2bin(b['beg'], b['end']) and a['ref'] == b['ref']
            for a, b in ((bam.records[k - 1], bam.records[k]) for k in range(7, len(bam.records), 7))]
    assert any(same) and not all(same)                                                                                # a run over a slab cut (of 7)
    bins = [M.reg2bin(r['beg'], r['end']) for r in bam.records if r['ref'] == 0]
    runs = [b for k, b in enumerate(bins) if k == 0 or bins[k - 1] != b]
    assert len(runs) > len(set(runs))                                                                                 # a bin that comes back
    data, _ = K.written(cases['block_end'], 1000, 'bai', zlib_blocks)
    bam = M.Bam(data)
    on_cut = [r for r in bam.records if r['stop'] % BLOCK == 0]
    assert len(on_cut) == 1 and bam.voffset(on_cut[0]['stop']) & 0xFFFF == 0 and bam.voffset(on_cut[0]['stop']) >> 16 == bam.members[1][0]
    data, _ = K.written(cases['edges'], 1000, 'bai', zlib_blocks)
    index, bam = M.parse(M.build(data, 'bai')[0]), M.Bam(data)
    by_name = dict(zip([ln.split('\t')[0] for ln in cases['edges']['text'].split('\n') if ln and ln[0] != '@'], bam.records))
    level = lambda r: M.reg2bin(r['beg'], r['end'])                  # noqa: E731
    assert 585 <= level(by_name['level4']) < 4681 and 73 <= level(by_name['level3']) < 585 and level(by_name['level0']) == 0
    assert by_name['three_windows']['end'] - 1 >> 14 == 2 and by_name['three_windows']['beg'] >> 14 == 0
    for name in ('no_cigar', 'all_insertion', 'placed_unmapped', 'placed_unmapped_cigar', 'pos0'):
        assert by_name[name]['end'] == by_name[name]['beg'] + 1
    assert by_name['pos0']['pos'] == -1 and by_name['pos0']['beg'] == 0
    assert index['refs'][1] == dict(bins={}, loffset={}, linear=[], meta=None)                                        # `empty`, between two
    assert index['refs'][0]['meta'][2:] == (sum(1 for r in bam.records if r['ref'] == 0 and not r['flag'] & 4), 3)
    assert by_name['chrM_overhang']['end'] > 16569 and len(index['refs'][3]['linear']) == 3 == (16569 + 16383 >> 14) + 1
    assert index['refs'][3]['linear'][2] == bam.voffset(by_name['chrM_overhang']['start'])
    assert index['n_no_coor'] == 3
    data, _ = K.written(cases['long_cigar'], 3, 'bai', zlib_blocks)
    assert M.Bam(data).records[1]['end'] == 19 + 32768
    data, _ = K.written(cases['header_only'], 3, 'csi', zlib_blocks)
    assert M.parse(M.build(data, 'csi')[0]) == dict(fmt='csi', depth=5, n_no_coor=0, refs=[dict(bins={}, loffset={}, linear=[], meta=None)] * 4)


@pytest.mark.parametrize('name,kind', [('edges', 'bai'), ('edges', 'csi'), ('many', 'bai'), ('many', 'csi'), ('block_end', 'bai'), ('big', 'csi'),
                                       ('long_cigar', 'bai')])
def test_every_record_is_found_and_every_chunk_begins_a_record(cases, name, kind):
    data, w = K.written(cases[name], 97, kind, zlib_blocks)
    index, bam = M.parse(_inflated(w)), M.Bam(data)
    depth = index['depth']
    placed = [r for r in bam.records if r['ref'] >= 0]
    assert placed and len(placed) + index['n_no_coor'] == len(bam.records)
    for r in placed:                                                 # none is left out
        v = bam.voffset(r['start'])
        assert any(c[0] <= v < c[1] for c in M.query(index, r['ref'], r['beg'], r['end'])), r
        if kind == 'bai':
            linear = index['refs'][r['ref']]['linear']
            assert linear[min(r['beg'] >> 14, len(linear) - 1)] <= v, r
    for ref, entry in enumerate(index['refs']):
        for b, chunks in entry['bins'].items():
            assert all(c[0] < c[1] for c in chunks) and all(x[1] <= y[0] for x, y in zip(chunks, chunks[1:]))
            for c in chunks:                                         # a seek to the chunk's begin lands on a record of the bin
                r = M.record_at(bam, c[0])
                assert r is not None and r['ref'] == ref and M.reg2bin(r['beg'], r['end'], 14, depth) == b, (ref, b, c)
        if entry['meta']:
            of_ref = [r for r in placed if r['ref'] == ref]
            assert entry['meta'] == (bam.voffset(of_ref[0]['start']), bam.voffset(of_ref[-1]['stop']),
                                     sum(1 for r in of_ref if not r['flag'] & 4), sum(1 for r in of_ref if r['flag'] & 4))


def test_the_chunk_merge_rule_is_at_work(cases):
    """A bin that comes back within one compressed block is one chunk: fewer chunks than runs."""
    data, w = K.written(cases['many'], 2000, 'bai', zlib_blocks)
    index = M.parse(w.index_data)
    chunks = sum(len(c) for entry in index['refs'] for c in entry['bins'].values())
    assert chunks < w.index_runs - 1                                 # (the runs count the reads without a coordinate as one)


def test_the_entry_point_refuses_what_does_not_fit(cases):
    from kbbq import _native as N
    lib = N.load()
    case = cases['edges']
    desc, skel, _ = C.layout(case['bam'], False, case['keep'])
    n = len(desc)
    lin_off = np.array([0, 4, 8, 12, 16], dtype=np.uint64)           # four windows a reference: every window index is clamped
    linear = np.full(16, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    runs = np.zeros(n * N.BAM_RUN_BYTES, dtype=np.uint8)
    count, bad = ctypes.c_int64(0), ctypes.c_int64(0)
    args = lambda d, depth=5, n_ref=4, cap=n, sk=skel.nbytes: (N.ptr(skel), sk, N.ptr(d), n, 1000, depth, N.ptr(lin_off), n_ref,  # noqa: E731
                                                               N.ptr(linear), N.ptr(runs), cap, ctypes.byref(count), ctypes.byref(bad))
    assert lib.kbbq_bam_index(*args(desc)) == N.KBBQ_OK and bad.value == -1 and 0 < count.value < n
    assert (linear != 0xFFFFFFFFFFFFFFFF).sum() >= 6 and linear[4:8].min() == 0xFFFFFFFFFFFFFFFF       # `empty` stays empty
    filled = linear.copy()
    linear[:] = 0xFFFFFFFFFFFFFFFF
    for broken_args, row in ((args(desc, n_ref=3), None), (args(desc, sk=int(desc[5, 0]) + 10), 5)):
        assert lib.kbbq_bam_index(*broken_args) == N.KBBQ_E_ARG and 'does not fit' in N.last_error()
        assert bad.value >= 0 and (row is None or bad.value == row) and count.value == 0
        assert np.all(linear == 0xFFFFFFFFFFFFFFFF)                  # nothing was touched
    short = desc.copy()
    short[7, 1] = 36                                                 # a head that ends before its QNAME and CIGAR
    assert lib.kbbq_bam_index(*args(short)) == N.KBBQ_E_ARG and bad.value == 7
    for bad_args in (args(desc, depth=4), args(desc, depth=9), args(desc, cap=n - 1), args(desc, n_ref=-1)):
        assert lib.kbbq_bam_index(*bad_args) == N.KBBQ_E_ARG
    assert lib.kbbq_bam_index_dev(None, *args(desc)) == N.KBBQ_E_ARG and 'ctx' in N.last_error()
    assert lib.kbbq_bam_index(*args(desc)) == N.KBBQ_OK and np.array_equal(linear, filled)
    assert N.BAM_RUN_BYTES == 32 == np.dtype(__import__('kbbq._bamindex', fromlist=['RUN']).RUN).itemsize


# ---------------------------------------------------------------- refusals, each before the output file exists
def _never(writer):
    raise AssertionError('the writer was opened')


def test_unsorted_input_is_refused_with_its_index(tmp_path):
    from kbbq import _bamindex
    from kbbq.gatk import applybqsr
    rng = np.random.default_rng(3)
    lines = K.edges(rng)
    k = 9
    lines[k - 1], lines[k] = lines[k], lines[k - 1]
    assert lines[k].split('\t')[3] != lines[k - 1].split('\t')[3]
    case = K.parsed(tmp_path, lines)
    out = tmp_path / 'never.bam'
    with pytest.raises(ValueError, match='alignment %d is out of coordinate order' % k) as err:
        applybqsr.write_bam_file(case['bam'], str(out), _never, index='auto')
    assert err.value.read_index == k
    assert not out.exists() and not (tmp_path / 'never.bam.bai').exists()
    # '*' sorts last: a read without a coordinate in front of a placed one is out of order; @HD SO: decides nothing
    lines = K.edges(rng)
    lines.insert(0, lines.pop())
    moved = K.parsed(tmp_path, lines, name='moved.sam')
    with pytest.raises(ValueError, match='alignment 1 is out of coordinate order') as err:
        _bamindex.check(moved['bam'], 5)
    assert err.value.read_index == 1
    _bamindex.check(moved['bam'], 5, 1)                              # the rest is in order
    unsorted_header = K.parsed(tmp_path, K.edges(rng), header=['@HD\tVN:1.6\tSO:unsorted'] + K.HEADER[1:], name='so.sam')
    _bamindex.check(unsorted_header['bam'], 5)
    # without the option the order of the records is nobody's business
    from kbbq import _bamout
    assert _bamout.check(case['bam']) is None and not out.exists()


def test_a_reference_too_long_for_bai_and_a_record_beyond_reach(tmp_path):
    from kbbq import _bamindex
    from kbbq.gatk import applybqsr
    rng = np.random.default_rng(4)
    case = K.parsed(tmp_path, K.big(rng), K.BIG)
    out = tmp_path / 'never.bam'
    with pytest.raises(ValueError, match=r'bai.*@SQ SN:wheat3B LN:536870913'):
        applybqsr.write_bam_file(case['bam'], str(out), _never, index='bai')
    assert not out.exists()
    assert _bamindex.resolve('auto', case['bam'].header) == ('csi', 6) and _bamindex.resolve('csi', case['bam'].header) == ('csi', 6)
    short = K.parsed(tmp_path, K.edges(rng), name='short.sam')
    assert _bamindex.resolve('auto', short['bam'].header) == ('bai', 5) == _bamindex.resolve('bai', short['bam'].header)
    assert _bamindex.resolve('csi', short['bam'].header) == ('csi', 5)
    # a record that ends beyond 2^(14 + 3 * depth): the @SQ line says 70000, the record lies past 2^29
    lines = [K.record(rng, 'in', 'small', 10), K.record(rng, 'out', 'small', (1 << 29) - 3, '10M'), K.record(rng, 'after', 'small', 1 << 29)]
    header = [ln for ln in K.BIG if 'wheat' not in ln]
    beyond = K.parsed(tmp_path, lines, header, name='beyond.sam')
    with pytest.raises(ValueError, match='alignment 1 ends beyond 2\\^29') as err:
        applybqsr.write_bam_file(beyond['bam'], str(out), _never, index='auto')
    assert err.value.read_index == 1 and not out.exists()
    with pytest.raises(ValueError, match='needs -o FILE'):
        applybqsr.write_bam_file(short['bam'], None, _never, index='auto')
    with pytest.raises(ValueError, match='one of auto, bai, csi'):
        applybqsr.write_bam_file(short['bam'], str(out), _never, index='tbi')
    assert not out.exists()


@pytest.mark.parametrize('argv', [['applybqsr', '-b', 'x.sam', '-g', 'r', '--bam-index', '-o', 'o.bam'],
                                  ['applybqsr', '-b', 'x.sam', '-g', 'r', '--bam-out', '--bam-index'],
                                  ['applybqsr', '-b', 'x.sam', '-g', 'r', '--bam-out', '--bam-index', 'csi'],
                                  ['applybqsr', '-b', 'x.sam', '-g', 'r', '--bam-out', '-o', 'o.bam', '--bam-index', 'tbi'],
                                  ['recalibrate', '-b', 'x.sam', '--kmers', '--bam-index', 'bai', '-o', 'o.bam'],
                                  ['recalibrate', '-b', 'x.sam', '--kmers', '--bam-out', '--bam-index'],
                                  ['recalibrate', '-b', 'x.sam', '--bam-out', '--bam-index', '-o', 'o.bam'],
                                  ['recalibrate', '-c', 'a.fq', '--bam-index', '-o', 'o.bam'],
                                  ['bqsr', '-b', 'x.sam', '--kmers', '-g', 'r', '--bam-index']])
def test_argparse_errors(argv, monkeypatch, capsys, tmp_path):
    from kbbq import main, parallel

    def never():
        raise AssertionError('the process group was touched')
    monkeypatch.setattr(parallel, 'init_from_env', never)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as err:
        main.main(argv)
    assert err.value.code == 2
    said = capsys.readouterr().err
    assert '--bam-index' in said or '--bam-out' in said
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize('given', [None, (), ('bai',), ('csi',), ('auto',)])
def test_the_option_goes_down_only_when_given(monkeypatch, tmp_path, given):
    from kbbq import main, parallel, recalibrate
    from kbbq.gatk import applybqsr
    seen = {}

    def fake(*args, **kw):
        seen.clear()
        seen.update(kw)
        return dict(k=31, min_count=2, reads=0, excluded_reads=0, flagged_bases=0, skipped_bases=0)
    monkeypatch.setattr(parallel, 'init_from_env', lambda: (1, 0))
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')
    for var in ('RANK', 'WORLD_SIZE'):
        monkeypatch.delenv(var, raising=False)
    flag = [] if given is None else ['--bam-index', *given]
    want = None if given is None else (given[0] if given else 'auto')
    monkeypatch.setattr(applybqsr, 'apply_report', fake)
    main.main(['applybqsr', '-b', 'x.sam', '-g', 'x.report', '--bam-out', '-o', 'out.bam'] + flag)
    assert seen.get('bam_index') == want and ('bam_index' in seen) == (given is not None) and seen['bam_out'] is True
    sam = tmp_path / 'x.sam'
    sam.write_text(C.sam_text([K.record(np.random.default_rng(1), 'a', 'chr1', 5)], K.HEADER))
    monkeypatch.setattr(main._recal, 'check_bam_records', lambda *a, **k: None)
    monkeypatch.setattr(recalibrate, 'recalibrate_bam', fake)
    main.main(['recalibrate', '-b', str(sam), '--kmers', '--bam-out', '-o', str(tmp_path / 'o.x')] + flag)
    assert seen.get('bam_index') == want and ('bam_index' in seen) == (given is not None)


def test_the_library_calls_refuse_the_option_without_its_company(tmp_path):
    from kbbq import recalibrate
    from kbbq.gatk import applybqsr
    with pytest.raises(ValueError, match='only with --bam-out'):
        applybqsr.apply_report('nowhere.sam', 'nowhere.report', output='x.sam', bam_index='auto')
    with pytest.raises(ValueError, match='needs -o FILE'):
        applybqsr.apply_report('nowhere.sam', 'nowhere.report', bam_out=True, bam_index='auto')
    with pytest.raises(ValueError, match='one of auto, bai, csi'):
        applybqsr.apply_report('nowhere.sam', 'nowhere.report', output='x.bam', bam_out=True, bam_index='tabix')
    with pytest.raises(ValueError, match='only with --bam-out'):
        recalibrate.check_bam_kmers('nowhere.sam', None, 'x.sam', bam_index='bai')
    with pytest.raises(ValueError, match='needs -o FILE'):
        recalibrate.check_bam_kmers('nowhere.sam', None, None, bam_out=True, bam_index='bai')
    recalibrate.check_bam_kmers('nowhere.sam', None, 'x.bam', bam_out=True, bam_index='csi')


def test_under_a_launcher_the_option_is_refused_before_the_group(monkeypatch, tmp_path):
    from kbbq import main, parallel
    monkeypatch.chdir(tmp_path)

    def never():
        raise AssertionError('the process group was joined')
    monkeypatch.setattr(parallel, 'init_from_env', never)
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '2')
    for argv in (['applybqsr', '-b', 'x.sam', '-g', 'r', '--bam-out', '--bam-index', '-o', 'o.bam'],
                 ['recalibrate', '-b', 'x.sam', '--kmers', '--bam-out', '--bam-index', 'csi', '-o', 'o.bam']):
        with pytest.raises(ValueError, match='SAM text path runs under ranks'):
            main.main(argv)
    assert os.listdir(tmp_path) == []


def test_the_index_file_is_written_beside_the_output_and_overwritten(cases, tmp_path):
    """open_sink(path, index=): path.bai / path.csi at close(), over whatever was there; none when the writer is left on an error."""
    from kbbq import _bamout
    case = cases['edges']
    bam, n = case['bam'], len(case['bam'])
    for kind, other in (('bai', 'csi'), ('csi', 'bai')):
        path = tmp_path / ('o.%s.bam' % kind)
        (tmp_path / (path.name + '.' + kind)).write_bytes(b'stale' * 10000)
        writer = _bamout.BamWriter(open(path, 'wb'), close_raw=True, deflate=zlib_blocks, index=kind, index_path=str(path))
        with writer as w:
            w.header(bam)
            w.records(bam.batch(), 0, n, False, case['keep'], case['seq'], case['out'], case['pitch'])
        made = (tmp_path / (path.name + '.' + kind)).read_bytes()
        assert made == w.index_data and not (tmp_path / (path.name + '.' + other)).exists()
        text = M.inflate(made) if kind == 'csi' else made
        assert text == M.build(path.read_bytes(), kind)[0]
    path = tmp_path / 'broken.bam'
    with pytest.raises(RuntimeError, match='midway'):
        with _bamout.BamWriter(open(path, 'wb'), close_raw=True, deflate=zlib_blocks, index='bai', index_path=str(path)) as w:
            w.header(bam)
            raise RuntimeError('midway')
    assert not (tmp_path / 'broken.bam.bai').exists()
    with pytest.raises(ValueError, match='records before the header'):
        with _bamout.BamWriter(open(path, 'wb'), close_raw=True, deflate=zlib_blocks, index='bai') as w:
            w.records(bam.batch(), 0, n, False, case['keep'], case['seq'], case['out'], case['pitch'])
