"""BAM recode without a GPU: the host twin of the recode kernels (kbbq_bam_recode: the same per-record code, csrc/kbbq_bam_recode.h
br_size / br_write) against the host route -- the reader on the BGZF file of the same image, then kbbq_bam_layout and
kbbq_bam_skeleton -- byte for byte on descriptors, skeleton and both sizes; the records it must flag; the damaged images of
tests/bam_in_cases.py; the refusals."""
import ctypes
import struct

import numpy as np
import pytest

import bam_in_cases as I
import bam_recode_cases as C


def _raw(img):
    return np.frombuffer(img, dtype=np.uint8)


def _scan(img):
    from kbbq import _bamin as B
    return B.Scan(_raw(img))


@pytest.mark.parametrize('name', C.ALL)
def test_host_twin_equals_the_host_route(name, tmp_path):
    """Every image, whole: set_oq in {0, 1} x keep in {none, all, alternating}."""
    img, flagged = C.named(name)
    scan = _scan(img)
    bam = C.reader(tmp_path, img, 'x')
    assert scan.n == len(bam)
    rules = C.expected_flags(bam, img, scan)
    assert flagged is None or flagged == rules
    flagged = rules
    assert (name in ('float', 'ref_below', 'in_hand_made', 'in_qualities', 'in_tags')) == bool(flagged)
    for set_oq in (0, 1):
        for kind, keep in C.keep_patterns(scan.n).items():
            got = C.recode_host(img, scan, 0, scan.n, set_oq, keep)
            C.assert_equals_host_route(got, C.reference(bam, 0, scan.n, set_oq, keep), flagged, (name, set_oq, kind))


@pytest.mark.parametrize('m', C.COUNTS)
def test_record_ranges(m, tmp_path):
    img, _ = C.named('many')
    scan = _scan(img)
    bam = C.reader(tmp_path, img, 'x')
    for first in (0, 311):
        for set_oq in (0, 1):
            keep = C.keep_patterns(m)['alternating']
            got = C.recode_host(img, scan, first, m, set_oq, keep)
            C.assert_equals_host_route(got, C.reference(bam, first, m, set_oq, keep), None, (first, m, set_oq))


def test_the_cases_hold_what_they_are_for():
    """The generators against their own claims."""
    from kbbq import _native as N
    img = C.image('int_types')
    for typ, (fmt, lo, hi) in C.INT_TYPES.items():
        for v in C.INT_EDGES:
            assert not lo <= v <= hi or b'XI' + typ.encode() + struct.pack(fmt, v) in img
    got = C.recode_host(img, _scan(img), 0, _scan(img).n, 0, None)
    assert got['skel_bytes'] < _scan(img).stream_bytes and got['any'] == 0                # (tags stored too wide shrink)
    places = C.image('int_places')
    for run in C.RUNS:
        assert ('run%d_front' % run).encode() in places or run == 0
    shapes = _scan(C.image('shapes'))
    lengths = [struct.unpack_from('<i', C.image('shapes'), int(o) + 16)[0] for o in shapes.rec_off]
    assert set(C.L_SEQS) <= set(lengths)
    assert all(struct.unpack_from('<H', C.image('shapes'), int(o) + 10)[0] == 4680 for o in shapes.rec_off)   # the stored bin
    got = C.recode_host(C.image('shapes'), shapes, 0, shapes.n, 0, None)
    bins = {struct.unpack_from('<H', got['skel'].tobytes(), int(d[0]) + 14)[0] for d in got['desc']}
    assert len(bins) > 3 and 4680 in bins                                                          # pos -1 -> 4680; the others differ
    assert N.BAM_ST_FLOAT == 32 and N.BAM_ST_REF == 64


@pytest.mark.parametrize('kind', I.CORRUPTIONS)
def test_damaged_records_end_with_the_decodes_status(kind):
    from kbbq import _bamin as B
    from kbbq import _native as N
    img, row, bit = I.corrupted(kind)
    scan = _scan(img)
    words = B.decode_host(_raw(img), scan, 32)['words']
    want = words[:, N.BAM_WORDS.index('status')].view(np.uint32)
    assert want[row] == bit and not want[[0, 2]].any()
    for set_oq in (0, 1):
        got = C.recode_host(img, scan, 0, scan.n, set_oq, np.array([1, 0, 1], np.uint8))
        assert got['rc'] == 0 and np.array_equal(got['status'], want) and got['any'] == bit
        assert not got['desc'][row][[1, 2, 3, 5]].any()
        # the neighbours are whole: block_size, then the record's own fixed bytes but for bin
        for r in (0, 2):
            off = int(got['desc'][r][0])
            body = int(scan.rec_off[r])
            assert got['skel'][off + 4:off + 14].tobytes() == img[body:body + 10]
    alone = C.recode_host(img, scan, row, 1, 1, None)
    assert alone['any'] == bit and alone['skel_bytes'] == 0 and alone['stream_bytes'] == 0


def test_offsets_outside_the_image_are_flagged_not_read():
    from kbbq import _native as N
    img = C.image('quals')
    scan = _scan(img)
    scan.rec_off = scan.rec_off.copy()
    scan.rec_off[1] = 2                                     # no room for a block_size word in front
    scan.rec_off[2] = len(img) + 1000
    scan.rec_off[3] = len(img) - 8                          # a block_size that runs past the image
    got = C.recode_host(img, scan, 0, 5, 1, None, cap=1 << 16)
    assert list(got['status']) == [0, N.BAM_ST_RANGE, N.BAM_ST_RANGE, N.BAM_ST_RANGE, 0] and got['any'] == N.BAM_ST_RANGE


def test_refusals(tmp_path):
    from kbbq import _native as N
    lib = N.load()
    img = C.image('quals')
    scan = _scan(img)
    raw, rec = _raw(img), np.ascontiguousarray(scan.rec_off, dtype=np.uint64)
    desc, status, skel = np.zeros((scan.n, 6), np.uint32), np.zeros(scan.n, np.uint32), np.zeros(1 << 16, np.uint8)
    sb, tb, st = ctypes.c_size_t(7), ctypes.c_size_t(7), ctypes.c_uint32(7)
    call = lambda first=0, m=scan.n, n_ref=3, d=desc, k=skel, cap=skel.nbytes, s=status, a=ctypes.byref(sb): lib.kbbq_bam_recode(  # noqa: E731
        N.ptr(raw), raw.nbytes, N.ptr(rec), first, m, 1, None, n_ref, N.ptr(d), N.ptr(k), cap, N.ptr(s), a, ctypes.byref(tb), ctypes.byref(st))
    assert call() == 0 and sb.value > 0 and st.value == 0
    for bad in (dict(first=-1), dict(m=-1), dict(m=2 ** 31), dict(n_ref=-1), dict(d=None), dict(s=None), dict(a=None), dict(k=None)):
        assert call(**bad) == -4, bad
        assert 'kbbq_bam_recode' in lib.kbbq_last_error().decode()
    # a skeleton that does not fit: the sizes are reported, the skeleton is not written
    small = np.full(64, C.POISON, np.uint8)
    assert call(k=small, cap=16) == -4 and sb.value > 16 and (small == C.POISON).all()
    # skel NULL with cap 0: sizes, descriptors and status words only
    whole = sb.value
    assert call(k=None, cap=0) == 0 and sb.value == whole
    want = C.reference(C.reader(tmp_path, img, 'x'), 0, scan.n, 1, None)
    assert np.array_equal(desc, want[0]) and whole == len(want[1]) and tb.value == want[2]
    assert call(m=0) == 0 and sb.value == 0 and tb.value == 0


def test_header_order_is_told_apart():
    """The @SQ lines of sq_reordered() name the binary list in another order: the route's check (kbbq._bamin.sq_lines_match)."""
    from kbbq import _bamin as B
    assert B.sq_lines_match(_scan(C.image('many'))) is None
    assert B.sq_lines_match(_scan(I.image('no_header_text'))) is None
    assert B.sq_lines_match(_scan(I.image('padded_header'))) is None
    assert B.sq_lines_match(_scan(C.sq_reordered())) == 'the @SQ lines do not name the binary reference list in order'


@pytest.mark.parametrize('name', ['many', 'in_padded_header', 'in_no_header_text', 'in_rg300', 'in_empty'])
def test_the_stream_head_from_header_lines_is_the_readers(name, tmp_path):
    """kbbq_bam_header_text on the scan's header lines against kbbq_bam_header on the reader: one statement, two ways in."""
    import bam_out_cases as O
    from kbbq import _native as N
    img, _ = C.named(name)
    want = O.header_bytes(C.reader(tmp_path, img, 'x'))
    text = np.frombuffer(''.join(line + '\n' for line in _scan(img).header).encode('latin-1'), dtype=np.uint8)
    need = ctypes.c_size_t(0)
    lib = N.load()
    N.check(lib.kbbq_bam_header_text(N.ptr(text) if text.nbytes else None, text.nbytes, None, 0, ctypes.byref(need)))
    head = np.zeros(need.value, np.uint8)
    N.check(lib.kbbq_bam_header_text(N.ptr(text) if text.nbytes else None, text.nbytes, N.ptr(head), head.nbytes, ctypes.byref(need)))
    assert head.tobytes() == want
    assert lib.kbbq_bam_header_text(N.ptr(text) if text.nbytes else None, text.nbytes, N.ptr(head), 3, ctypes.byref(need)) == -4
    bad = np.frombuffer(b'@SQ\tSN:x\n', dtype=np.uint8)
    assert lib.kbbq_bam_header_text(N.ptr(bad), bad.nbytes, None, 0, ctypes.byref(need)) == -5


def test_host_twin_under_the_sanitizers(tmp_path):
    """tests/native/bam_recode_sanitize.cpp: every buffer a heap block of exactly the size the interface names -- the skeleton of
    exactly the bytes the size step measured; the images of this suite, the damaged records, and images cut short."""
    import os
    import subprocess
    from conftest import ROOT
    exe = str(tmp_path / 'bam_recode_sanitize')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-o', exe,
                           os.path.join(ROOT, 'tests', 'native', 'bam_recode_sanitize.cpp')])
    images = {name: C.named(name)[0] for name in C.ALL if name != 'in_trims'}
    images.update({kind: I.corrupted(kind)[0] for kind in I.CORRUPTIONS})
    images['cut'] = C.image('quals')[:-3]
    files = []
    for name, img in images.items():
        files.append(str(tmp_path / (name + '.img')))
        with open(files[-1], 'wb') as fh:
            fh.write(img)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    for set_oq in (0, 1):
        r = subprocess.run([exe, str(set_oq)] + files, capture_output=True, timeout=300, env=env)
        out, err = r.stdout.decode('latin-1'), r.stderr.decode('latin-1')
        assert 'ERROR: AddressSanitizer' not in err and 'runtime error' not in err, err[-3000:]
        assert r.returncode == 0, (r.returncode, err[-2000:])
        lines = out.strip().split('\n')
        assert len(lines) == len(files)
        for (name, img), said in zip(images.items(), lines):
            if name == 'cut':
                assert said.endswith(' scan: BAM: truncated record')
                continue
            scan = _scan(img)
            got = C.recode_host(img, scan, 0, scan.n, set_oq, (np.arange(scan.n) % 2).astype(np.uint8))
            total = sum(int(got[key].view(np.uint8).sum(dtype=np.uint64)) for key in ('desc', 'status', 'skel'))
            assert said.endswith(' n=%d status=%d skel=%d stream=%d sum=%d' % (scan.n, got['any'], got['skel_bytes'], got['stream_bytes'], total)), (name, said)
