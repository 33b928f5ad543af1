"""Test infrastructure of --bam-out: SAM records that cover what the BAM encoder has to tell apart, the SAM text T that defines
the stream (kbbq_sam_render with given QUAL rows), and the stream as the host entry points make it (kbbq_bam_header + kbbq_bam_layout
+ kbbq_bam_skeleton + kbbq_bam_assemble)."""
import ctypes

import numpy as np

HEADER = ['@HD\tVN:1.6\tSO:unsorted', '@SQ\tSN:chr1\tLN:248956422', '@SQ\tSN:chr2\tLN:242193529', '@SQ\tSN:chrM\tLN:16569',
          '@RG\tID:rg0\tPU:pu0\tSM:s', '@RG\tID:rg1\tPU:pu1\tSM:s', '@RG\tID:rg2\tPU:pu2\tSM:s', '@CO\ta comment\twith a tab']

INT_EDGES = [-2 ** 31, -32769, -32768, -129, -128, -1, 0, 127, 128, 255, 256, 32767, 32768, 65535, 65536, 2 ** 31 - 1, 2 ** 31,
             2 ** 32 - 1]


def _qual(rng, n):
    return ''.join(chr(33 + int(q)) for q in rng.integers(2, 41, n))


def _seq(rng, n, letters='ACGT'):
    return ''.join(letters[int(i)] for i in rng.integers(0, len(letters), n))


def hand_made(rng):
    """Records chosen for the encoder's cases (every one a line BAM can hold)."""
    s10, q10 = _seq(rng, 10), _qual(rng, 10)
    lines = []

    def rec(name, flag=0, rname='chr1', pos=100, mapq=60, cigar=None, rnext='=', pnext=200, tlen=150, seq=s10, qual=q10, tags=()):
        if cigar is None:
            cigar = '%dM' % len(seq) if seq != '*' else '*'
        lines.append('\t'.join([name, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual, *tags]))
    rec('plain', tags=['RG:Z:rg0'])
    for k, v in enumerate(INT_EDGES):                                    # integer tags at every type boundary
        rec('int%d' % k, tags=['RG:Z:rg%d' % (k % 3), 'XI:i:%d' % v, 'NM:i:%d' % (k % 5)])
    rec('types', tags=['RG:Z:rg1', 'XA:A:Q', 'XF:f:1.5', 'XG:f:-0.25', 'XE:f:3e+10', 'XZ:Z:a string, with: colons', 'XY:Z:', 'XH:H:1AE301',
                       'OQ:Z:' + _qual(rng, 10)])
    rec('arrays', tags=['RG:Z:rg2', 'Bc:B:c,-128,0,127', 'BC:B:C,0,255', 'Bs:B:s,-32768,32767', 'BS:B:S,0,65535,7',
                        'Bi:B:i,-2147483648,2147483647', 'BI:B:I,0,4294967295', 'Bf:B:f,0.5,-2,0.001', 'B0:B:c'])
    rec('unmapped', flag=4, rname='*', pos=0, mapq=0, cigar='*', rnext='*', pnext=0, tlen=0, tags=['RG:Z:rg0'])
    rec('mate_elsewhere', flag=65, rnext='chr2', pnext=5000, tlen=0, tags=['RG:Z:rg0'])
    rec('mate_unplaced', flag=73, rnext='*', pnext=0, tlen=0, tags=['RG:Z:rg1'])
    rec('mate_named_same', flag=65, rname='chr2', rnext='chr2', tags=['RG:Z:rg1'])
    rec('chrM', rname='chrM', pos=16560, tags=['RG:Z:rg2'])
    rec('no_cigar', cigar='*', tags=['RG:Z:rg0'])
    rec('ops', cigar='2S3M1I1M1D1M1N1=1X5H2P', seq=s10, tags=['RG:Z:rg0'])
    rec('long_span', pos=16383, cigar='5M40000N5M', tags=['RG:Z:rg0'])              # the bin leaves the finest level
    rec('far', pos=200000000, cigar='5M3000000N5M', tags=['RG:Z:rg0'])
    rec('no_seq', cigar='*', seq='*', qual='*', tags=['RG:Z:rg0'])
    rec('no_qual', qual='*', tags=['RG:Z:rg1'])
    rec('no_qual_oq', qual='*', tags=['RG:Z:rg1', 'OQ:Z:' + _qual(rng, 10)])
    rec('iupac', seq='=ACMGRSVTWYHKDBN', qual=_qual(rng, 16), tags=['RG:Z:rg2'])
    rec('iupac_odd', seq='NBDKHYWTVSRGMCA', qual=_qual(rng, 15), tags=['RG:Z:rg2'])
    rec('one_base', seq='G', qual='I', tags=['RG:Z:rg0'])
    rec('no_tags')
    rec('n' * 254, tags=['RG:Z:rg0'])                                                # the longest QNAME
    rec('empty_tag_field', tags=['RG:Z:rg0', '', 'NM:i:3'])
    rec('reverse_mate', flag=147, pos=3000, pnext=2800, tlen=-210, tags=['RG:Z:rg1', 'MD:Z:10'])
    return lines


def random_records(rng, n, lo=1, hi=70, p_no_oq=0.15, p_star=0.03, name='r'):
    """n records of lengths lo..hi over the three read groups; some without an OQ tag, some with QUAL '*'."""
    lines = []
    for i in range(n):
        L = int(rng.integers(lo, hi + 1))
        flag = int(rng.choice([0, 16, 99, 147, 83, 163]))
        qual = '*' if rng.random() < p_star else _qual(rng, L)
        tags = ['RG:Z:rg%d' % int(rng.integers(0, 3)), 'NM:i:%d' % int(rng.integers(0, 300))]
        if rng.random() >= p_no_oq:
            tags.append('OQ:Z:' + _qual(rng, L))
        if rng.random() < 0.3:
            tags.append('XS:i:%d' % int(rng.integers(-70000, 70000)))
        lines.append('\t'.join(['%s%d' % (name, i), str(flag), 'chr%d' % int(rng.integers(1, 3)), str(int(rng.integers(1, 10 ** 6))),
                                str(int(rng.integers(0, 61))), '%dM' % L, '=', str(int(rng.integers(1, 10 ** 6))),
                                str(int(rng.integers(-500, 500))), _seq(rng, L), qual, *tags]))
    return lines


def sam_text(lines, header=HEADER):
    return ''.join(x + '\n' for x in list(header) + list(lines))


def planes(bam, rng, keep=None):
    """(seq plane, QUAL plane, keep mask, pitch) of an aln.AlignmentFile: new QUAL characters at random for the records that take
    them, the QUAL as read for those of `keep` (default: every fifth record) and for '*'."""
    b = bam.batch()
    n = len(bam)
    pitch = max(16, (int(b.maxlen) + 15) // 16 * 16)
    seq, qual = b.plane(0, pitch), b.plane(1, pitch)
    if keep is None:
        keep = np.arange(n) % 5 == 4
    keep = np.asarray(keep, dtype=bool) | (b.qual_len == 0)
    out = rng.integers(33, 33 + 60, (max(n, 1), pitch)).astype(np.uint8)
    out[:n][keep] = qual[:n][keep]
    return seq, out, keep, pitch


def rendered(bam, out, pitch, set_oq, first=0, n=None, header=True):
    """T: the header lines as read and the alignment lines with their QUAL replaced by the rows of `out` (kbbq_sam_render)."""
    from kbbq import _native as N
    lib = N.load()
    n = len(bam) - first if n is None else n
    need = ctypes.c_size_t(0)
    N.check(lib.kbbq_sam_render(bam.batch()._native, first, n, N.ptr(out), pitch, int(set_oq), None, 0, ctypes.byref(need)))
    buf = np.empty(max(need.value, 1), dtype=np.uint8)
    N.check(lib.kbbq_sam_render(bam.batch()._native, first, n, N.ptr(out), pitch, int(set_oq), N.ptr(buf), buf.nbytes, ctypes.byref(need)))
    head = ''.join(x + '\n' for x in bam.header) if header else ''
    return head + buf[:need.value].tobytes().decode('latin-1')


def header_bytes(bam):
    from kbbq import _native as N
    lib = N.load()
    need = ctypes.c_size_t(0)
    N.check(lib.kbbq_bam_header(bam.batch()._native, None, 0, ctypes.byref(need)))
    head = np.empty(need.value, dtype=np.uint8)
    N.check(lib.kbbq_bam_header(bam.batch()._native, N.ptr(head), head.nbytes, ctypes.byref(need)))
    return head.tobytes()


def layout(bam, set_oq, keep, first=0, n=None):
    """(descriptors [n, 6], skeleton bytes, stream size) of alignments [first, first + n)."""
    from kbbq import _native as N
    lib = N.load()
    n = len(bam) - first if n is None else n
    desc = np.zeros((max(n, 1), N.BAM_DESC_WORDS), dtype=np.uint32)
    keep8 = None if keep is None else np.ascontiguousarray(keep[first:first + n], dtype=np.uint8)
    skel_bytes, stream_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    N.check(lib.kbbq_bam_layout(bam.batch()._native, first, n, int(set_oq), N.ptr(keep8), N.ptr(desc), ctypes.byref(skel_bytes),
                                ctypes.byref(stream_bytes)))
    skel = np.zeros(max(skel_bytes.value, 1), dtype=np.uint8)
    N.check(lib.kbbq_bam_skeleton(bam.batch()._native, first, n, int(set_oq), N.ptr(desc), N.ptr(skel), skel_bytes.value))
    return desc[:n], skel[:skel_bytes.value], stream_bytes.value


def host_stream(bam, seq, out, pitch, set_oq, keep):
    """The record part of the stream by the host entry points, and the lowest row with a quality below 0 (-1: none)."""
    from kbbq import _native as N
    desc, skel, size = layout(bam, set_oq, keep)
    stream = np.zeros(max(size, 1), dtype=np.uint8)
    bad = ctypes.c_int64(-1)
    N.check(N.load().kbbq_bam_assemble(N.ptr(skel), skel.nbytes, N.ptr(desc), len(desc), N.ptr(seq), N.ptr(out), pitch, N.ptr(stream), 0,
                                       size, ctypes.byref(bad)))
    return stream[:size].tobytes(), int(bad.value)
