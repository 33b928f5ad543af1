"""Test infrastructure of BAM input (include/kbbq_hip.h "BAM input"): inflated BAM images that cover what the decode has to tell
apart, the corrupted images every status bit answers, and the comparison of a decode with the host reader on the same bytes.
The reference throughout is kbbq.aln.AlignmentFile on the BGZF file of the image, never the code under test."""
import functools
import struct

import numpy as np

import bamwriter
from bam_out_cases import HEADER, hand_made, random_records, sam_text

LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 150, 151, 4097, 65535]
COUNTS = [1, 15, 16, 17, 255, 256, 257]
IUPAC = '=ACMGRSVTWYHKDBN'
REFS = [('chr1', 248956422), ('chr2', 242193529), ('chrM', 16569)]


def _qual(rng, n):
    return ''.join(chr(33 + int(q)) for q in rng.integers(0, 94, n))          # every quality BAM and the text both hold


def _seq(rng, n):
    return ''.join(IUPAC[int(i)] for i in rng.integers(0, 16, n))


def line(name, seq, qual, tags=(), flag=0, rname='chr1', pos=100, cigar=None, rnext='=', pnext=200, tlen=150):
    if cigar is None:
        cigar = '%dM' % len(seq) if seq != '*' else '*'
    return '\t'.join([name, str(flag), rname, str(pos), '60', cigar, rnext, str(pnext), str(tlen), seq, qual, *tags])


# ---- records built directly as bytes (what SAM text cannot say) ------------------------------------------------------------------
def raw_record(name=b'raw', flag=0, ref_id=0, pos=99, ops=(), next_ref=0, pnext=199, tlen=150, seq='ACGT', qual=None, tags=b'',
               l_seq=None, l_name=None):
    n = len(seq)
    packed = bytearray((n + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= bamwriter.SEQ[c] << (4 if i % 2 == 0 else 0)
    qual = bytes([30] * n) if qual is None else qual
    qname = name + b'\0'
    body = struct.pack('<iiBBHHHiiii', ref_id, pos, len(qname) if l_name is None else l_name, 60, 4680, len(ops), flag,
                       n if l_seq is None else l_seq, next_ref, pnext, tlen)
    body += qname + b''.join(struct.pack('<I', o) for o in ops) + bytes(packed) + qual + tags
    return struct.pack('<i', len(body)) + body


def raw_image(records, header=HEADER, refs=REFS, header_text=True):
    htext = (''.join(x + '\n' for x in header)).encode('latin-1') if header_text else b''
    out = [b'BAM\1', struct.pack('<i', len(htext)), htext, struct.pack('<i', len(refs))]
    for name, ln in refs:
        out += [struct.pack('<i', len(name) + 1), name.encode() + b'\0', struct.pack('<i', ln)]
    return b''.join(out) + b''.join(records)


def z(tag, value):
    return tag + b'Z' + value + b'\0'


# ---- the cases: name -> inflated image ------------------------------------------------------------------------------------------
def _lengths(rng):
    """Every length of LENGTHS (all 16 nibble codes among them) with the OQ variants in turn: absent, as long as SEQ, shorter,
    longer than SEQ (and so than the pitch), empty, two OQ tags."""
    lines = []
    for k, L in enumerate(LENGTHS * 2):
        seq = _seq(rng, L) if L else '*'
        if L >= 16:
            seq = IUPAC + seq[16:]
        ql = lambda m: _qual(rng, min(m, 32767))                               # (32767: the longest value the reader's arrays hold)
        oq = [[], ['OQ:Z:' + ql(L)], ['OQ:Z:' + ql(max(L - 3, 0))], ['OQ:Z:' + ql(L + 40)], ['OQ:Z:'],
              ['OQ:Z:' + ql(5), 'XX:i:1', 'OQ:Z:' + ql(L)]][(k + k // len(LENGTHS)) % 6]
        qual = _qual(rng, L) if L and k % 5 != 3 else '*'
        if L == 1 and qual == '*':
            qual = '+'
        lines.append(line('len%d_%d' % (L, k), seq, qual, ['RG:Z:rg%d' % (k % 3)] + oq, cigar='*' if not L else None))
    return bamwriter.sam_to_bam_bytes(sam_text(lines))


def _qualities(rng):
    recs = [raw_record(b'present', seq='ACGTACGTACGTACGTACG', qual=bytes(range(75, 94)), tags=z(b'RG', b'rg0')),
            raw_record(b'absent', seq='ACGTACGTACGTACGTACG', qual=b'\xff' * 19, tags=z(b'RG', b'rg1')),
            raw_record(b'ff_first', seq='ACGTACGTACGTACGTACG', qual=b'\xff' + bytes(range(18)), tags=z(b'RG', b'rg2')),
            raw_record(b'ff_later', seq='ACGT', qual=b'\x05\x06\x07\x08', tags=z(b'RG', b'rg0')),
            raw_record(b'one_base_q9', seq='G', qual=b'\x09', tags=z(b'RG', b'rg0')),       # renders as '*': "no QUAL" in the text
            raw_record(b'one_base_q10', seq='G', qual=b'\x0a', tags=z(b'RG', b'rg0')),
            raw_record(b'q93', seq='ACGTACGTACGTACGTA', qual=b'\x5d' * 17, tags=z(b'RG', b'rg0')),
            raw_record(b'neg_ref', ref_id=-1, next_ref=-1, pos=-1, pnext=-1, tlen=0, flag=4, tags=z(b'RG', b'rg0')),
            raw_record(b'neg_ref2', ref_id=-7, next_ref=-3, flag=4, tags=z(b'RG', b'rg0')),
            raw_record(b'', seq='AC', tags=z(b'RG', b'rg0'))]                              # an empty QNAME
    return raw_image(recs)


def _read_groups(n_rg):
    def image(rng):
        header = ['@HD\tVN:1.6', '@SQ\tSN:chr1\tLN:1000000'] + ['@RG\tID:g%d\tPU:p%d' % (g, g) for g in range(n_rg)]
        if n_rg > 2:
            header += ['@RG\tID:g1\tPU:again', '@RG\tPU:no_id', '@RG\tID:a\tID:b\tPU:two_ids', '@RG\tID:\tPU:short']
        names = ['g%d' % g for g in (0, n_rg - 1, n_rg // 2)] + ['g1', 'b', 'a', 'nowhere', 'g', 'g00']
        lines = [line('known%d' % k, 'ACGTACGT', 'IIIIIIII', ['NM:i:1', 'RG:Z:' + g]) for k, g in enumerate(names)]
        lines += [line('absent', 'ACGT', 'IIII', ['NM:i:2']),
                  line('two', 'ACGT', 'IIII', ['RG:Z:nowhere', 'XA:A:q', 'RG:Z:g0']),
                  line('two_last_unknown', 'ACGT', 'IIII', ['RG:Z:g0', 'RG:Z:nowhere']),
                  line('empty_value', 'ACGT', 'IIII', ['RG:Z:']),
                  line('not_z', 'ACGT', 'IIII', ['RG:A:x']),
                  line('not_z_then_z', 'ACGT', 'IIII', ['RG:Z:g0', 'RG:A:x']),
                  line('hex', 'ACGT', 'IIII', ['RG:H:1A', 'OQ:H:2B'])]
        return bamwriter.sam_to_bam_bytes(sam_text(lines, header))
    return image


def _tags(rng):
    """Tags of every type in front of RG / OQ: each skip length is exercised."""
    ahead = ['XA:A:Q', 'Xc:i:-5', 'XC:i:200', 'Xs:i:-3000', 'XS:i:60000', 'Xi:i:-100000', 'XI:i:4000000000', 'Xf:f:1.5', 'XZ:Z:a string',
             'XE:Z:', 'XH:H:1AE301', 'Bc:B:c', 'BC:B:C', 'Bs:B:s', 'BS:B:S', 'Bi:B:i', 'BI:B:I', 'Bf:B:f',
             'bc:B:c,' + ','.join(str(int(v)) for v in rng.integers(-128, 128, 37)),
             'bC:B:C,' + ','.join(str(int(v)) for v in rng.integers(0, 256, 41)),
             'bs:B:s,' + ','.join(str(int(v)) for v in rng.integers(-32768, 32768, 33)),
             'bS:B:S,' + ','.join(str(int(v)) for v in rng.integers(0, 65536, 35)),
             'bi:B:i,' + ','.join(str(int(v)) for v in rng.integers(-2 ** 31, 2 ** 31, 29)),
             'bI:B:I,' + ','.join(str(int(v)) for v in rng.integers(0, 2 ** 32, 31)),
             'bf:B:f,' + ','.join('%g' % v for v in rng.normal(size=27))]
    lines = []
    for k, tag in enumerate(ahead):
        L = 10 + k
        lines.append(line('tag%d' % k, _seq(rng, L), _qual(rng, L), [tag, 'RG:Z:rg%d' % (k % 3), tag[:1] + 'y' + tag[2:], 'OQ:Z:' + _qual(rng, L)]))
    lines.append(line('all', _seq(rng, 40), _qual(rng, 40), ahead + ['RG:Z:rg1', 'OQ:Z:' + _qual(rng, 40)]))
    for pad in range(9):                                                       # the NUL of a Z value at every position of a dword
        lines.append(line('z%d' % pad, 'ACGT', 'IIII', ['XZ:Z:' + 'v' * pad, 'RG:Z:rg2', 'YZ:Z:' + 'w' * (pad + 3)]))
    return bamwriter.sam_to_bam_bytes(sam_text(lines))


def _cigars(rng):
    lines = [line('nine', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='2S3M1I1M1D1M1N1=1X5H2P'),
             line('hard_outside', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='7H2S5M3S9H'),
             line('hard_only_lead', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='4H10M'),
             line('soft_inside', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='3M2S3M2S'),
             line('all_soft', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='10S'),
             line('none', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='*'),
             line('one', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='10M'),
             line('wide', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='5M268435455N5M'),          # the span clamps at INT32_MAX
             line('wide2', 'ACGTACGTAC', _qual(rng, 10), ['RG:Z:rg0'], cigar='268435455D' * 9 + '10M'),
             line('long_clip', 'ACGT', _qual(rng, 4), ['RG:Z:rg0'], cigar='70000S4M70000S')]
    head = bamwriter.sam_to_bam_bytes(sam_text(lines))
    # n_cigar_op is a 16-bit field: 65535 operations is the most a record holds; with the next record's 4465 the file has 70000
    many = [(int(l) << 4) | int(o) for l, o in zip(rng.integers(1, 9, 65535), rng.integers(0, 9, 65535))]
    more = [(int(l) << 4) | int(o) for l, o in zip(rng.integers(1, 9, 4465), rng.integers(0, 9, 4465))]
    return head + raw_record(b'many', ops=many, flag=99, tlen=400, tags=z(b'RG', b'rg1')) \
                + raw_record(b'more', ops=more, flag=147, pos=5000, pnext=3000, tlen=-2500, tags=z(b'RG', b'rg2')) \
                + raw_record(b'after', ops=[(4 << 4)], tags=z(b'RG', b'rg0'))


def _trims(rng):
    """The random pairs of tests/test_oracle_bqsr.py::test_native_adaptor_trim_is_the_per_read_walk: every operation, short
    inserts, both strands, mates unmapped."""
    lines = []
    for i in range(3000):
        ops, q = [], 0
        for k in range(int(rng.integers(1, 7))):
            op = 'MIDNS=X'[int(rng.integers(0, 7))] if k else 'MS=X'[int(rng.integers(0, 4))]
            l = int(rng.integers(1, 12))
            ops.append((l, op)); q += l if op in 'MIS=X' else 0
        if q == 0 or not any(op in 'M=X' for _, op in ops):
            ops.append((5, 'M')); q += 5
        span = sum(l for l, op in ops if op in 'MDN=X')
        pos = int(rng.integers(1, 500))
        flag = int(rng.choice([99, 147, 83, 163] * 3 + [67, 115, 73, 97, 0, 16, 1 | 16 | 8, 4 | 1 | 32]))
        pnext = max(1, pos + int(rng.integers(-span - 5, span + 6)))
        tlen = int(rng.integers(-span - 8, span + 9))
        qual = '*' if i % 97 == 5 else 'I' * q
        lines.append(line('r%d' % i, 'A' * q, qual, ['RG:Z:rg0', 'OQ:Z:' + 'I' * q], flag=flag, pos=pos,
                          cigar=''.join('%d%s' % o for o in ops), pnext=pnext, tlen=tlen))
    return bamwriter.sam_to_bam_bytes(sam_text(lines))


def _count(n):
    return lambda rng: bamwriter.sam_to_bam_bytes(sam_text(random_records(rng, n)))


def _no_header_text(rng):
    return bamwriter.sam_to_bam_bytes(sam_text(random_records(rng, 40)), header_text=False)


def _padded_header(rng):
    """NUL padding behind the header text, no line end at its end, a '\\r' before a line end, a blank line."""
    htext = '@HD\tVN:1.6\r\n\n@SQ\tSN:chr1\tLN:1000\n \t\n@RG\tID:rg0\tPU:x\n@CO\tlast'.encode() + b'\0' * 7
    img = [b'BAM\1', struct.pack('<i', len(htext)), htext, struct.pack('<i', 1), struct.pack('<i', 5), b'chr1\0', struct.pack('<i', 1000)]
    return b''.join(img) + raw_record(b'a', tags=z(b'RG', b'rg0')) + raw_record(b'b', ref_id=-1, next_ref=-1)


def _empty(rng):
    return bamwriter.sam_to_bam_bytes(sam_text([]))


CASES = dict([('hand_made', lambda rng: bamwriter.sam_to_bam_bytes(sam_text(hand_made(rng)))), ('lengths', _lengths),
              ('qualities', _qualities), ('rg1', _read_groups(1)), ('rg300', _read_groups(300)), ('tags', _tags), ('cigars', _cigars),
              ('trims', _trims), ('no_header_text', _no_header_text), ('padded_header', _padded_header), ('empty', _empty)]
             + [('count%d' % n, _count(n)) for n in COUNTS])


@functools.lru_cache(maxsize=None)
def image(name):
    """The case's inflated image (bytes), made once."""
    return CASES[name](np.random.default_rng(sum(name.encode()) + 7))


def slab_cuts(name):
    """slab_bytes values for a case: the default (one slab), a cut after every record, after every 3 records or so, and one that
    leaves a record larger than the slab."""
    return [None, 1, 1000, 40000]


# ---- the corrupted images: kind -> (image, row of the damaged record, status bit) ---------------------------------------------------
def corrupted(kind):
    """Three records, the middle one damaged in the image; its neighbours must come out exact."""
    from kbbq import _native as N
    tags = z(b'XZ', b'abc') + z(b'RG', b'rg1') + z(b'OQ', b'I' * 19)
    good = dict(seq='ACGTACGTACGTACGTACG', qual=bytes(range(20, 39)), ops=[(19 << 4)], tags=tags)
    mid = dict(good)
    bit = N.BAM_ST_RECORD
    if kind == 'qual94':
        mid['qual'] = bytes(range(20, 38)) + b'\x5e'; bit = N.BAM_ST_QUAL
    elif kind == 'qual94_first_chunk':
        mid['qual'] = b'\x14\x5e' + bytes(range(22, 39)); bit = N.BAM_ST_QUAL
    elif kind == 'rg_tab':
        mid['tags'] = z(b'RG', b'rg\t1') + z(b'OQ', b'I' * 19); bit = N.BAM_ST_TEXT
    elif kind == 'oq_space':
        mid['tags'] = z(b'RG', b'rg1') + z(b'OQ', b'I' * 17 + b' I'); bit = N.BAM_ST_TEXT
    elif kind == 'z_newline':
        mid['tags'] = z(b'XZ', b'a\nb') + z(b'RG', b'rg1'); bit = N.BAM_ST_TEXT
    elif kind == 'qname_tab':
        mid['name'] = b'a\tb'; bit = N.BAM_ST_TEXT
    elif kind == 'cigar_op9':
        mid['ops'] = [(19 << 4) | 9]; bit = N.BAM_ST_TEXT
    elif kind == 'l_name0':
        mid['l_name'] = 0
    elif kind == 'b_count':
        mid['tags'] = b'XBBc' + struct.pack('<I', 2 ** 31 - 1) + b'\1\2' + z(b'RG', b'rg1')
    elif kind == 'b_subtype':
        mid['tags'] = b'XBBq' + struct.pack('<I', 1) + b'\1' + z(b'RG', b'rg1')
    elif kind == 'l_seq_negative':
        mid['l_seq'] = -1
    elif kind == 'l_seq_huge':
        mid['l_seq'] = 2 ** 31 - 1
    elif kind == 'tag_cut':
        mid['tags'] = z(b'RG', b'rg1') + b'OQZIIII'                           # no NUL before the record's end
    elif kind == 'tag_cut_int':
        mid['tags'] = z(b'RG', b'rg1') + b'XIi\1\2'
    elif kind == 'tag_type':
        mid['tags'] = b'XXq\1' + z(b'RG', b'rg1')
    elif kind == 'next_ref':
        mid['next_ref'] = len(REFS)
    elif kind == 'ref_id':
        mid['ref_id'] = len(REFS)
    elif kind == 'qname_no_nul':
        mid['name'] = None
    else:
        raise KeyError(kind)
    if mid.get('name', b'') is None:
        rec = bytearray(raw_record(b'mid', **{k: v for k, v in mid.items() if k != 'name'}))
        rec[4 + 32 + 3] = ord('x')                                             # the NUL of QNAME
        rec = bytes(rec)
    else:
        rec = raw_record(mid.pop('name', b'mid'), **mid)
    return raw_image([raw_record(b'before', **good), rec, raw_record(b'after', **good)]), 1, bit


CORRUPTIONS = ['qual94', 'qual94_first_chunk', 'rg_tab', 'oq_space', 'z_newline', 'qname_tab', 'cigar_op9', 'l_name0', 'b_count',
               'b_subtype', 'l_seq_negative', 'l_seq_huge', 'tag_cut', 'tag_cut_int', 'tag_type', 'next_ref', 'ref_id', 'qname_no_nul']

# what the scan refuses, with the reader's words
SCAN_ERRORS = {
    'not a BAM file': lambda img: img[:10],               # (another magic is SAM text to the reader: it never sees the BAM route)
    'BAM header text runs past the file': lambda img: img[:4] + struct.pack('<i', len(img)) + img[8:],
    'BAM reference list runs past the file': lambda img: img[:12 + struct.unpack('<i', img[4:8])[0] + 6],
    'BAM: negative reference count': lambda img: (lambda at: img[:at] + struct.pack('<i', -2) + img[at + 4:])(8 + struct.unpack('<i', img[4:8])[0]),
    'BAM: truncated record': lambda img: img[:-3],
}


# ---- the comparison ----------------------------------------------------------------------------------------------------------------
def reader(tmp_path, img, name='x'):
    """The host reader on the BGZF file of the image."""
    from kbbq import aln
    path = tmp_path / (name + '.bam')
    path.write_bytes(bamwriter.bgzf(img))
    return aln.AlignmentFile(str(path)), str(path)


WORDS = ('flag', 'pos', 'pnext', 'tlen', 'qlen', 'qual_len', 'oq_len', 'rg', 'cig_n', 'ref_span', 'clip')


def assert_equals_reader(got, scan, ref, pitches_checked):
    """got: kbbq._bamin.decode_host's dict (or the device's in that form) at pitch got['pitch']; ref: the reader."""
    from kbbq import _native as N
    b = ref.batch()
    assert scan.n == b.n and got['status'] == 0
    col = {name: got['words'][:, k] for k, name in enumerate(N.BAM_WORDS)}
    for name in WORDS:
        want = getattr(b, name)
        have = col[name].view(np.uint32) if want.dtype == np.uint32 else col[name]
        assert np.array_equal(have.astype(np.int64), want.astype(np.int64)), name
    assert np.array_equal(col['trim'].view(np.uint32), b.adaptor_trim()), 'trim'
    assert not col['status'].any() and not col['pad0'].any() and not col['pad1'].any()
    assert np.array_equal(scan.cig_off[:b.n].astype(np.uint32), b.cig_off) and scan.cig_total == len(b.cigar)
    assert np.array_equal(got['cigar'], b.cigar), 'cigar'
    names = ['*' if r < 0 else scan.ref_names[r] for r in col['ref_id']]
    assert names == [b.contig_names[c] for c in b.contig], 'contig'
    pitch = got['pitch']
    for which, plane in enumerate(('seq', 'qual', 'oq')):
        if b.n:
            assert np.array_equal(got[plane], b.plane(which, pitch)[:b.n]), (plane, pitch)
    pitches_checked.add(pitch)
