"""Test infrastructure of the BAM recode (include/kbbq_hip.h "BAM recode"): inflated BAM images, built record by record with
bam_in_cases.raw_record / raw_image, that cover what the recode has to tell apart, the call with poisoned and guarded outputs, and
the comparison with the host route.  The reference throughout is kbbq.aln.AlignmentFile on the BGZF file of the same image, then
kbbq_bam_layout / kbbq_bam_skeleton (bam_out_cases.layout) -- never the recode itself."""
import ctypes
import functools
import struct

import numpy as np

import bam_in_cases as I
import bam_out_cases as O
import bamwriter
from bam_in_cases import raw_image, raw_record, z

INT_EDGES = O.INT_EDGES
INT_TYPES = {'c': ('<b', -128, 127), 'C': ('<B', 0, 255), 's': ('<h', -32768, 32767), 'S': ('<H', 0, 65535),
             'i': ('<i', -2 ** 31, 2 ** 31 - 1), 'I': ('<I', 0, 2 ** 32 - 1)}
RUNS = [0, 4, 15, 16, 17, 33]                # total bytes of a tail that go over unchanged (a whole tag has at least four: no run of 1)
COUNTS = [1, 15, 16, 17, 255, 256, 257]
L_SEQS = [0, 1, 2, 15, 16, 17, 151]
POISON, GUARD = 0xA5, 64


def itag(name, typ, value):
    return name + typ.encode() + struct.pack(INT_TYPES[typ][0], value)


def barray(name, sub, values):
    return name + b'B' + sub.encode() + struct.pack('<I', len(values)) + b''.join(struct.pack(INT_TYPES[sub][0], v) for v in values)


def zrun(n, name=b'ZZ'):
    """A Z tag of n bytes in all (n >= 4)."""
    return z(name, b'v' * (n - 4))


def _seq(rng, n):
    return ''.join('ACGT'[int(i)] for i in rng.integers(0, 4, n))


def _qual(rng, n):
    return bytes(int(q) for q in rng.integers(2, 41, n))


def _rec(rng, name, L=20, **kw):
    kw.setdefault('seq', _seq(rng, L))
    kw.setdefault('qual', _qual(rng, len(kw['seq'])))
    if 'ops' not in kw and len(kw['seq']):
        kw['ops'] = [(len(kw['seq']) << 4)]
    return raw_record(name.encode(), **kw)


# ---- the cases: name -> records ---------------------------------------------------------------------------------------------------
def _int_types(rng):
    """Every storage type with every boundary value it holds: stored minimally, and stored too wide."""
    recs = []
    for typ, (_, lo, hi) in INT_TYPES.items():
        for v in INT_EDGES:
            if lo <= v <= hi:
                recs.append(_rec(rng, '%s_%d' % (typ, v), tags=z(b'RG', b'rg0') + itag(b'XI', typ, v)))
    return recs


def _int_places(rng):
    """Integer tags (too wide: 'i' holding 5, 'C' holding 7, 'S' holding 300) first, last, adjacent, between long Z values; tails
    whose unchanged bytes are RUNS in all."""
    wide = [itag(b'Xa', 'i', 5), itag(b'Xb', 'C', 7), itag(b'Xc', 'S', 300), itag(b'Xd', 'I', 70000), itag(b'Xe', 's', -3)]
    long_z = z(b'ZL', b'l' * 77)
    recs = [_rec(rng, 'first', tags=wide[0] + long_z),
            _rec(rng, 'last', tags=long_z + wide[1]),
            _rec(rng, 'adjacent', tags=long_z + wide[0] + wide[1] + wide[2] + long_z),
            _rec(rng, 'between', tags=long_z + wide[3] + z(b'ZM', b'm' * 130) + wide[4] + long_z),
            _rec(rng, 'minimal_between', tags=itag(b'Xm', 'c', 5) + wide[2] + itag(b'Xn', 'S', 40000) + wide[0] + itag(b'Xo', 'I', 2 ** 31))]
    for run in RUNS:
        for k, where in enumerate(('front', 'middle', 'back', 'split')):
            if run == 0:
                tags = wide[0] + wide[1] + wide[2]
            elif where == 'front':
                tags = zrun(run) + wide[0] + wide[1]
            elif where == 'middle':
                tags = wide[0] + zrun(run) + wide[1]
            elif where == 'back':
                tags = wide[0] + wide[1] + zrun(run)
            elif run >= 8:
                tags = zrun(run // 2, b'ZA') + wide[0] + zrun(run - run // 2, b'ZB')
            else:
                continue
            recs.append(_rec(rng, 'run%d_%s' % (run, where), L=20 + k, tags=tags))
    return recs


def _other_tags(rng):
    recs = []
    for sub, (_, lo, hi) in INT_TYPES.items():
        for count in (0, 1, 17):
            values = [lo, hi] * 9
            recs.append(_rec(rng, 'B%s_%d' % (sub, count), tags=barray(b'XB', sub, values[:count]) + itag(b'Xw', 'i', 1)))
    recs += [_rec(rng, 'A', tags=b'XAAq' + itag(b'Xw', 'I', 2)),
             _rec(rng, 'H', tags=b'XHH1AE3\0' + itag(b'Xw', 'S', 3)),
             _rec(rng, 'empty_Z', tags=z(b'XZ', b'') + itag(b'Xw', 's', 4)),
             _rec(rng, 'two_OQ', tags=z(b'OQ', b'I' * 5) + itag(b'Xw', 'i', -1) + z(b'OQ', b'J' * 20)),
             _rec(rng, 'empty_OQ', tags=z(b'OQ', b'')),
             _rec(rng, 'OQ_not_Z', tags=b'OQAx' + b'OQH1A\0'),
             _rec(rng, 'no_tags', tags=b'')]
    return recs


def _quals(rng):
    """QUAL present, 0xFF throughout, 0xFF followed by other bytes, ONE quality of 9 -- each without an OQ tag and with one."""
    recs = []
    for k, oq in enumerate((b'', z(b'OQ', b'I' * 19))):
        s, one = 'ACGTACGTACGTACGTACG', (z(b'OQ', b'I') if oq else b'')
        recs += [_rec(rng, 'present%d' % k, seq=s, qual=bytes(range(60, 79)), tags=oq),
                 _rec(rng, 'absent%d' % k, seq=s, qual=b'\xff' * 19, tags=oq),
                 _rec(rng, 'ff_first%d' % k, seq=s, qual=b'\xff' + bytes(range(18)), tags=oq),
                 _rec(rng, 'one_q9_%d' % k, seq='G', qual=b'\x09', tags=one),
                 _rec(rng, 'one_q10_%d' % k, seq='G', qual=b'\x0a', tags=one),
                 _rec(rng, 'q93_%d' % k, seq=s, qual=b'\x5d' * 19, tags=oq)]
    return recs


def _shapes(rng):
    recs = []
    for L in L_SEQS:
        recs.append(_rec(rng, 'L%d' % L, L=L, tags=z(b'RG', b'rg1') + itag(b'NM', 'i', L)))
        recs.append(_rec(rng, 'L%d_no_qual' % L, seq=_seq(rng, L), qual=b'\xff' * L, tags=z(b'RG', b'rg1')))
    ops = [(int(l) << 4) | int(o) for l, o in zip(rng.integers(1, 9, 1000), rng.integers(0, 9, 1000))]
    recs += [_rec(rng, 'bin_far', pos=5_000_000, tags=z(b'RG', b'rg0')),                # (raw_record stores bin 4680 in every record)
             _rec(rng, 'bin_span', pos=16380, ops=[(20 << 4), (100000 << 4) | 3, (5 << 4)], seq=_seq(rng, 25)),
             _rec(rng, 'next_same', ref_id=1, next_ref=1),
             _rec(rng, 'next_other', ref_id=0, next_ref=2),
             _rec(rng, 'next_none', ref_id=2, next_ref=-1, pnext=-1, tlen=0),
             _rec(rng, 'unmapped', ref_id=-1, next_ref=-1, pos=-1, pnext=-1, tlen=0, flag=4, ops=[]),
             _rec(rng, 'unmapped_mate_placed', ref_id=-1, next_ref=1, pos=-1, pnext=500, tlen=0, flag=5, ops=[]),
             _rec(rng, 'pos_minus_1', ref_id=0, pos=-1),
             _rec(rng, 'no_cigar', ops=[]),
             _rec(rng, 'many_ops', ops=ops, seq=_seq(rng, 30)),
             _rec(rng, 'long_name_' + 'n' * 230),
             raw_record(b'', seq='AC', ops=[(2 << 4)])]
    return recs


def _many(rng):
    """600 records of mixed lengths and tags, for the record ranges."""
    recs = []
    for k in range(600):
        L = int(rng.integers(1, 70))
        tags = z(b'RG', b'rg%d' % (k % 3))
        if k % 3:
            tags += itag(b'NM', 'iCcS'[k % 4], int(rng.integers(0, 100)))
        if k % 7:
            tags += z(b'OQ', bytes(33 + int(q) for q in rng.integers(2, 41, L)))
        if k % 11 == 0:
            tags += barray(b'XB', 's', [int(v) for v in rng.integers(-300, 300, k % 5)])
        qual = b'\xff' * L if k % 13 == 5 else _qual(rng, L)
        recs.append(_rec(rng, 'r%d' % k, seq=_seq(rng, L), qual=qual, tags=tags, pos=int(rng.integers(0, 100000)), ref_id=k % 3,
                         next_ref=(k // 2) % 3))
    return recs


VOUCHED = dict(int_types=_int_types, int_places=_int_places, other_tags=_other_tags, quals=_quals, shapes=_shapes, many=_many)


# records the recode must flag: name -> (records, {row: bit name})
def _float(rng):
    f = b'XFf' + struct.pack('<f', 0.1)
    return [_rec(rng, 'before'), _rec(rng, 'f', tags=z(b'RG', b'rg0') + f), _rec(rng, 'between', tags=itag(b'Xw', 'i', 3)),
            _rec(rng, 'Bf', tags=b'XGBf' + struct.pack('<Iff', 2, 1.5, 1e-7)), _rec(rng, 'Bf_empty', tags=b'XGBf' + struct.pack('<I', 0)),
            _rec(rng, 'after', tags=z(b'XZ', b'z'))], {1: 'BAM_ST_FLOAT', 3: 'BAM_ST_FLOAT', 4: 'BAM_ST_FLOAT'}


def _ref_below(rng):
    return [_rec(rng, 'before'), _rec(rng, 'ref', ref_id=-2, next_ref=-1, flag=4), _rec(rng, 'next', ref_id=0, next_ref=-9),
            _rec(rng, 'after', ref_id=-1, next_ref=-1, flag=4)], {1: 'BAM_ST_REF', 2: 'BAM_ST_REF'}


FLAGGED = dict(float=_float, ref_below=_ref_below)


@functools.lru_cache(maxsize=None)
def image(name):
    rng = np.random.default_rng(sum(name.encode()) + 11)
    if name in VOUCHED:
        return raw_image(VOUCHED[name](rng))
    return raw_image(FLAGGED[name](rng)[0])


def flagged_rows(name):
    from kbbq import _native as N
    return {row: getattr(N, bit) for row, bit in FLAGGED[name](np.random.default_rng(0))[1].items()}


def expected_flags(bam, img, scan):
    """{row: bit} of an image by the rules alone, from the reader's lines (a tag field of type f or B:f) and the stored refIDs
    (one below -1) -- not from the recode."""
    from kbbq import _native as N
    out = {}
    for r in range(scan.n):
        fields = bam.batch().line(r).split('\t')[11:]
        bit = N.BAM_ST_FLOAT if any(f[3:5] == 'f:' or f[3:7] == 'B:f,' or f[3:] == 'B:f' for f in fields) else 0
        ref, nxt = struct.unpack_from('<i', img, int(scan.rec_off[r]))[0], struct.unpack_from('<i', img, int(scan.rec_off[r]) + 20)[0]
        bit |= N.BAM_ST_REF if ref < -1 or nxt < -1 else 0
        if bit:
            out[r] = bit
    return out


def sq_reordered():
    """An image whose @SQ lines name the binary reference list in another order."""
    header = [O.HEADER[0], O.HEADER[2], O.HEADER[1]] + O.HEADER[3:]
    return raw_image(_many(np.random.default_rng(3))[:40], header=header)


def keep_patterns(n):
    return {'none': None, 'all': np.ones(n, np.uint8), 'alternating': (np.arange(n) % 2).astype(np.uint8)}


# ---- the call, with poisoned outputs between guards -----------------------------------------------------------------------------------
def skel_cap(scan, first, m, set_oq):
    """An upper bound of the skeleton of records [first, first + m): their bytes in the image, and an OQ tag each with set_oq."""
    if m == 0:
        return 0
    end = int(scan.rec_off[first + m]) - 4 if first + m < scan.n else scan.image_bytes
    return end - (int(scan.rec_off[first]) - 4) + (m * (scan.maxlen + 4) if set_oq else 0)


def guarded(nbytes):
    """(the whole buffer, poisoned; the offset of the payload)."""
    return np.full(GUARD + int(nbytes) + GUARD, POISON, np.uint8), GUARD


def result(desc_buf, status_buf, skel_buf, m, cap, skel_bytes, stream_bytes, any_status, rc):
    """The outputs out of their guarded buffers (host copies); asserts that nothing around them was touched."""
    for buf, used in ((desc_buf, 24 * m), (status_buf, 4 * m), (skel_buf, skel_bytes if rc == 0 else 0)):
        assert (buf[:GUARD] == POISON).all() and (buf[GUARD + used:] == POISON).all(), 'a byte outside the outputs was written'
    assert skel_bytes <= cap or rc != 0
    return dict(desc=desc_buf[GUARD:GUARD + 24 * m].view(np.uint32).reshape(m, 6).copy(), status=status_buf[GUARD:GUARD + 4 * m].view(np.uint32).copy(),
                skel=skel_buf[GUARD:GUARD + (skel_bytes if rc == 0 else 0)].copy(), skel_bytes=skel_bytes, stream_bytes=stream_bytes,
                any=any_status, rc=rc)


def recode_host(img, scan, first, m, set_oq, keep, cap=None):
    """kbbq_bam_recode on records [first, first + m) of the image."""
    from kbbq import _native as N
    raw = np.frombuffer(img, dtype=np.uint8)
    cap = skel_cap(scan, first, m, set_oq) if cap is None else cap
    (desc, at), (status, _), (skel, _) = guarded(24 * m), guarded(4 * m), guarded(cap)
    rec_off = np.ascontiguousarray(scan.rec_off, dtype=np.uint64)
    keep8 = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    sb, tb, any_status = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0)
    rc = N.load().kbbq_bam_recode(N.ptr(raw), raw.nbytes, N.ptr(rec_off), first, m, int(set_oq), N.ptr(keep8), scan.n_ref, N.ptr(desc[at:]),
                                  N.ptr(skel[at:]), cap, N.ptr(status[at:]), ctypes.byref(sb), ctypes.byref(tb), ctypes.byref(any_status))
    return result(desc, status, skel, m, cap, sb.value, tb.value, any_status.value, rc)


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def reference(bam, first, m, set_oq, keep):
    """The host route's (descriptors, skeleton, stream size) of alignments [first, first + m) of the reader; keep: of those m."""
    full = None
    if keep is not None:
        full = np.zeros(len(bam), np.uint8)
        full[first:first + m] = keep
    return O.layout(bam, set_oq, full, first, m)


def _piece(desc_row, skel):
    off, head, tail, l_seq, _, src = (int(v) for v in desc_row)
    return skel[off:off + head + (l_seq if src == 1 else 0) + tail].tobytes()


def assert_equals_host_route(got, want, flagged=None, what=None):
    """got: result(); want: reference().  Without flagged rows everything is equal byte for byte.  With them ({row: bit}): their
    status is the bit, their descriptors are zeros but for the offsets, they take no room, and every other record's descriptor
    fields and skeleton bytes are the reference's."""
    desc, skel, stream = want
    flagged = flagged or {}
    assert got['rc'] == 0, what
    m = len(desc)
    assert np.array_equal(got['status'], np.array([flagged.get(r, 0) for r in range(m)], np.uint32)), what
    bits = 0
    for b in flagged.values():
        bits |= b
    assert got['any'] == bits, what
    if not flagged:
        assert np.array_equal(got['desc'], desc), what
        assert got['skel'].tobytes() == skel.tobytes(), what
        assert (got['skel_bytes'], got['stream_bytes']) == (len(skel), stream), what
        return
    at_skel = at_stream = 0
    for r in range(m):
        g = got['desc'][r]
        assert (int(g[0]), int(g[4])) == (at_skel, at_stream), (what, r)
        if r in flagged:
            assert not g[[1, 2, 3, 5]].any(), (what, r)
            continue
        assert np.array_equal(g[[1, 2, 3, 5]], desc[r][[1, 2, 3, 5]]), (what, r)
        piece = _piece(g, got['skel'])
        assert piece == _piece(desc[r], skel), (what, r)
        at_skel += len(piece)
        at_stream += int(g[1]) + (int(g[3]) + 1) // 2 + int(g[3]) + int(g[2])
    assert (got['skel_bytes'], got['stream_bytes']) == (at_skel, at_stream), what


def reader(tmp_path, img, name):
    return I.reader(tmp_path, img, name)[0]


ALL = [name for name in VOUCHED] + [name for name in FLAGGED] + ['in_' + name for name in I.CASES]


def named(name):
    """(image, {row: bit} for the cases made to be flagged, None for the others: expected_flags says)."""
    if name.startswith('in_'):
        return I.image(name[3:]), None
    return image(name), (flagged_rows(name) if name in FLAGGED else {})


def bgzf_file(tmp_path, img, name='x'):
    path = tmp_path / (name + '.bam')
    path.write_bytes(bamwriter.bgzf(img))
    return str(path)
