"""BAM input without a GPU: the scan of an inflated image (kbbq_bam_scan) and the host twin of the decode kernel (kbbq_bam_decode:
the same per-record code, csrc/kbbq_bam_in.h bd_record) against the host reader on the same BAM bytes -- every array, every plane
byte at two pitches, the header lines -- over the cases of tests/bam_in_cases.py and every slab cut; the status records; the scan's
refusals in the reader's words; when aln.alignments stays with the reader; and both under the sanitizers in a program of their own."""
import os
import subprocess

import numpy as np
import pytest

import bam_in_cases as C
from conftest import ROOT


def _pitch_for(n):
    return max(16, (int(n) + 15) // 16 * 16)


def _raw(img):
    return np.frombuffer(img, dtype=np.uint8)


@pytest.mark.parametrize('name', list(C.CASES))
def test_scan_and_host_twin_equal_the_reader(name, tmp_path):
    from kbbq import _bamin as B
    img = C.image(name)
    ref, _ = C.reader(tmp_path, img)
    b = ref.batch()
    scan = B.Scan(_raw(img))
    assert scan.header == list(ref.header) and scan.header_ok
    assert scan.rg_ids == b.rg_ids and scan.n == b.n and scan.maxlen == b.maxlen
    checked = set()
    full = _pitch_for(max(b.maxlen, 1))
    for pitch, cuts in ((full, C.slab_cuts(name)), (32 if full != 32 else 16, [None, 1000])):
        for slab_bytes in cuts:
            got = B.decode_host(_raw(img), scan, pitch, slab_bytes)
            got['pitch'] = pitch
            C.assert_equals_reader(got, scan, ref, checked)
    assert len(checked) == 2


def test_the_cases_hold_what_they_are_for(tmp_path):
    """The generators against their own claims: every length and count, every nibble code, the QUAL and OQ kinds, the tag types."""
    from kbbq import _bamin as B
    lengths = C.reader(tmp_path, C.image('lengths'))[0].batch()
    assert set(C.LENGTHS) <= set(int(x) for x in lengths.qlen)
    assert set(lengths.plane(0, 16)[lengths.qlen >= 16][0].tobytes().decode()) == set(C.IUPAC)
    oq, q = lengths.oq_len, lengths.qlen
    assert (oq < 0).any() and (oq == q).any() and ((oq >= 0) & (oq < q)).any() and (oq > q).any() and (oq == 0).any()
    quals = C.reader(tmp_path, C.image('qualities'), 'q')[0].batch()
    assert list(quals.qual_len[:6]) == [19, 0, 0, 4, 0, 1]
    for n in C.COUNTS:
        assert B.Scan(_raw(C.image('count%d' % n))).n == n
    assert len(C.reader(tmp_path, C.image('rg300'), 'g')[0].batch().rg_ids) == 304 and B.Scan(_raw(C.image('rg1'))).rg_ids == ['g0']
    rg = C.reader(tmp_path, C.image('rg300'), 'g')[0].batch().rg
    assert (rg == -1).any() and (rg == -2).any() and (rg == 1).any() and (rg == 299).any() and (rg == 302).any()
    tags = C.image('tags')
    for t in b'AcCsSiIfZH':
        assert b'X' + bytes([t]) + bytes([t]) in tags                                                # tag X<t> of type <t>
    for sub in b'cCsSiIf':
        assert b'B' + bytes([sub]) + b'B' + bytes([sub]) + b'\0\0\0\0' in tags                       # an array of no elements
    cig = C.reader(tmp_path, C.image('cigars'), 'c')[0].batch()
    assert int(cig.cig_n.max()) == 65535 and int(cig.cig_n.sum()) > 70000 and set(int(x) & 15 for x in cig.cigar) == set(range(9))
    trims = C.reader(tmp_path, C.image('trims'), 't')[0].batch().adaptor_trim()
    assert int(((trims >> 16) > (trims & 0xFFFF)).sum()) > 300


def test_slabs_are_cut_at_record_boundaries():
    from kbbq import _bamin as B
    img = C.image('lengths')
    scan = B.Scan(_raw(img))
    assert [s[:2] for s in B.slabs(scan, 1)] == [(i, i + 1) for i in range(scan.n)]
    for slab_bytes in (1000, 40000, None):
        cuts = B.slabs(scan, slab_bytes)
        assert cuts[0][0] == 0 and cuts[-1][1] == scan.n and cuts[-1][3] == len(img) and cuts[0][2] == scan.records_off
        assert all(a[1] == b[0] and a[3] == b[2] for a, b in zip(cuts, cuts[1:]))
        limit = slab_bytes or B.stage_bytes()
        assert all(hi - lo <= limit or b - a == 1 for a, b, lo, hi in cuts)
        if slab_bytes == 40000:
            assert any(hi - lo > limit for _, _, lo, hi in cuts) and any(b - a > 3 for a, b, _, _ in cuts)


@pytest.mark.parametrize('kind', C.CORRUPTIONS)
def test_a_damaged_record_is_flagged_writes_zeros_and_leaves_its_neighbours_exact(kind, tmp_path):
    from kbbq import _bamin as B
    from kbbq import _native as N
    img, row, bit = C.corrupted(kind)
    clean = C.raw_image([C.raw_record(b'before', seq='ACGTACGTACGTACGTACG', qual=bytes(range(20, 39)), ops=[(19 << 4)],
                                      tags=C.z(b'XZ', b'abc') + C.z(b'RG', b'rg1') + C.z(b'OQ', b'I' * 19))] * 2)
    ref = C.reader(tmp_path, clean)[0].batch()
    scan = B.Scan(_raw(img))
    assert scan.n == 3
    status_at = N.BAM_WORDS.index('status')
    for pitch in (32, 16):
        for slab_bytes in (None, 1):
            got = B.decode_host(_raw(img), scan, pitch, slab_bytes)
            assert got['status'] == bit and int(got['words'][row, status_at]) == bit
            assert not got['words'][row, :status_at].any() and not got['words'][row, status_at + 1:].any()
            for which, plane in enumerate(('seq', 'qual', 'oq')):
                assert not got[plane][row].any(), plane
                assert np.array_equal(got[plane][[0, 2]], ref.plane(which, pitch)[:2]), plane
            lo, hi = int(scan.cig_off[row]), int(scan.cig_off[row + 1])
            assert hi - lo == 1 and not got['cigar'][lo:hi].any()
            assert np.array_equal(np.delete(got['cigar'], np.s_[lo:hi]), ref.cigar)
            for k, name in enumerate(N.BAM_WORDS[:11]):
                if name != 'ref_id':
                    assert np.array_equal(got['words'][[0, 2], k].astype(np.int64), getattr(ref, name).astype(np.int64)), name


def test_a_cigar_range_that_is_not_the_records_is_refused_not_written():
    """The caller's cig_off decides what may be written: a range of another size than n_cigar_op, or one past cig_cap."""
    import ctypes
    from kbbq import _bamin as B
    from kbbq import _native as N
    img = _raw(C.image('count17'))
    scan = B.Scan(img)
    lo = int(scan.rec_off[0]) - 4
    piece = np.ascontiguousarray(img[lo:])
    rec, cig = B._slab_tables(scan, 0, scan.n, lo)
    words = np.zeros((scan.n, 16), np.int32)
    status_at = N.BAM_WORDS.index('status')
    for damage in ('size', 'cap', 'order', 'record'):
        c, r, cap = cig.copy(), rec.copy(), int(cig[-1])
        if damage == 'size':
            c[5:] += 1
            cap += 1
        elif damage == 'cap':
            cap -= 1
        elif damage == 'order':
            c[4] = c[5] + 1
        else:
            r[4] = piece.nbytes + 5
        ops = np.full(int(c[-1]) + 2, 0xA5A5A5A5, np.uint32)
        any_status = ctypes.c_uint32(0)
        N.check(N.load().kbbq_bam_decode(N.ptr(piece), piece.nbytes, N.ptr(r), scan.n, 32, N.ptr(scan.rg_off), N.ptr(scan.rg_bytes),
                                         len(scan.rg_ids), scan.n_ref, N.ptr(c), cap, None, None, None, N.ptr(words), N.ptr(ops),
                                         ctypes.byref(any_status)))
        assert any_status.value == N.BAM_ST_RANGE, damage
        flagged = np.flatnonzero(words[:, status_at])
        assert list(flagged) == {'size': [4], 'cap': [scan.n - 1], 'order': [3, 4], 'record': [4]}[damage], damage
        assert (ops[int(c[-1]):] == 0xA5A5A5A5).all() and (ops[:cap][ops[:cap] != 0xA5A5A5A5] >> 4).max() < 71


@pytest.mark.parametrize('message', list(C.SCAN_ERRORS))
def test_a_scan_error_is_the_readers_message(message, tmp_path):
    from kbbq import _bamin as B
    from kbbq import aln
    bad = C.SCAN_ERRORS[message](C.image('hand_made'))
    with pytest.raises(ValueError) as scan_says:
        B.Scan(_raw(bad))
    assert str(scan_says.value) == message
    path = tmp_path / 'bad.bam'
    path.write_bytes(C.bamwriter.bgzf(bad))
    with pytest.raises(ValueError) as reader_says:
        aln.AlignmentFile(str(path))
    assert str(reader_says.value) == '%s: %s' % (path, message)


def test_entry_points_refuse_bad_arguments():
    import ctypes
    from kbbq import _native as N
    lib = N.load()
    slab = np.zeros(64, np.uint8)
    off = np.zeros(1, np.uint32)
    st = ctypes.c_uint32(7)
    plane = np.zeros(64, np.uint8)
    base = plane.ctypes.data
    for kw in (dict(pitch=24), dict(pitch=0), dict(m=-1), dict(slab=None), dict(seq=base + 1 if base % 16 == 0 else base), dict(status=None),
               dict(n_rg=1), dict(cigar=True)):
        ops = np.zeros(4, np.uint32)
        with pytest.raises(ValueError):
            N.check(lib.kbbq_bam_decode(None if 'slab' in kw else N.ptr(slab), slab.nbytes, N.ptr(off), kw.get('m', 1), kw.get('pitch', 16), None, None,
                                        kw.get('n_rg', 0), 1, None, 0, ctypes.c_void_p(kw['seq']) if 'seq' in kw else None, None, None, None,
                                        N.ptr(ops) if 'cigar' in kw else None, None if 'status' in kw else ctypes.byref(st)))
    with pytest.raises(ValueError):
        N.check(lib.kbbq_bam_scan(None, 12, None, None, None, None, None, None))
    with pytest.raises(ValueError):
        N.check(lib.kbbq_bam_decode_dev(None, N.ptr(slab), slab.nbytes, N.ptr(off), 1, 16, None, None, 0, 1, None, 0, None, None, None, None, None,
                                        ctypes.byref(st)))


def test_alignments_stays_with_the_reader_unless_asked(tmp_path, monkeypatch):
    """Default OFF; text, a launcher's rank and a file that is no BGZF stay with the reader before any device call."""
    from kbbq import aln
    monkeypatch.delenv('KBBQ_GPU_BAM', raising=False)
    ref, path = C.reader(tmp_path, C.image('count17'))
    got = aln.alignments(path)
    assert type(got) is aln.AlignmentFile and aln.LAST_RUN['bam_in'] == dict(route='host', records=17, stream_bytes=0, h2d_bytes=0, slabs=0,
                                                                            fallback='not asked for')
    sam = tmp_path / 'x.sam'
    sam.write_text(C.sam_text(C.random_records(np.random.default_rng(3), 5)))
    got = aln.alignments(str(sam), device=True)
    assert type(got) is aln.AlignmentFile and aln.LAST_RUN['bam_in']['fallback'] == 'not a BGZF file' and len(got) == 5
    monkeypatch.setenv('KBBQ_GPU_BAM', '1')
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '2')
    got = aln.alignments(path)
    assert type(got) is aln.AlignmentFile and aln.LAST_RUN['bam_in']['fallback'] == 'a rank of a launcher'
    assert aln.LAST_RUN['bam_in']['route'] == 'host' and np.array_equal(got.batch().flag, ref.batch().flag)
    assert issubclass(aln.DeviceAlignments, aln.AlignmentFile)


def test_scan_and_host_twin_under_the_sanitizers(tmp_path):
    """tests/native/bam_in_sanitize.cpp: every buffer a heap block of exactly the size the interface names; the well-formed cases,
    the damaged records, the scan errors, and images cut short at every kind of place."""
    from kbbq import _bamin as B
    exe = str(tmp_path / 'bam_in_sanitize')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-o', exe,
                           os.path.join(ROOT, 'tests', 'native', 'bam_in_sanitize.cpp')])
    images = {name: C.image(name) for name in C.CASES if name != 'trims'}
    images.update({kind: C.corrupted(kind)[0] for kind in C.CORRUPTIONS})
    images.update({'scan%d' % k: fn(C.image('hand_made')) for k, fn in enumerate(C.SCAN_ERRORS.values())})
    files = []
    for name, img in images.items():
        files.append(str(tmp_path / (name + '.img')))
        with open(files[-1], 'wb') as fh:
            fh.write(img)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    for pitch, slab_bytes in ((32, 1000), (160, 1 << 30)):
        r = subprocess.run([exe, str(pitch), str(slab_bytes)] + files, capture_output=True, timeout=300, env=env)
        out, err = r.stdout.decode('latin-1'), r.stderr.decode('latin-1')
        assert 'ERROR: AddressSanitizer' not in err and 'runtime error' not in err, err[-3000:]
        assert r.returncode == 0, (r.returncode, err[-2000:])
        lines = out.strip().split('\n')
        assert len(lines) == len(files)
        for (name, img), said in zip(images.items(), lines):
            if name.startswith('scan'):
                assert ' scan: ' in said and said.split(' scan: ')[1] in C.SCAN_ERRORS
                continue
            scan = B.Scan(_raw(img))
            got = B.decode_host(_raw(img), scan, pitch, slab_bytes)
            total = sum(int(got[p].sum(dtype=np.uint64)) for p in ('seq', 'qual', 'oq')) if scan.n else 0
            total += int(got['words'].view(np.uint8).sum(dtype=np.uint64)) + int(got['cigar'].view(np.uint8).sum(dtype=np.uint64))
            assert said.endswith(' n=%d status=%d sum=%d' % (scan.n, got['status'], total)), (name, said)
