"""Test infrastructure of --bam-index: coordinate-sorted SAM records at the smallest shapes at which an index can go wrong, and
kbbq/_bamout.py's BamWriter driven over them slab by slab (the host twin and a zlib stand-in, or the GPU)."""
import io

import numpy as np

import bam_out_cases as C
import bamwriter

BLOCK = 65280
HEADER = ['@HD\tVN:1.6\tSO:coordinate', '@SQ\tSN:chr1\tLN:248956422', '@SQ\tSN:empty\tLN:5000', '@SQ\tSN:chr2\tLN:242193529',
          '@SQ\tSN:chrM\tLN:16569', '@RG\tID:rg0\tPU:pu0\tSM:s', '@RG\tID:rg1\tPU:pu1\tSM:s', '@RG\tID:rg2\tPU:pu2\tSM:s']
BIG = ['@HD\tVN:1.6\tSO:coordinate', '@SQ\tSN:small\tLN:70000', '@SQ\tSN:wheat3B\tLN:%d' % ((1 << 29) + 1),
       '@RG\tID:rg0\tPU:pu0\tSM:s', '@RG\tID:rg1\tPU:pu1\tSM:s', '@RG\tID:rg2\tPU:pu2\tSM:s']


def record(rng, name, rname, pos, cigar=None, L=None, flag=0, tags=('RG:Z:rg0',), qual=None):
    """One SAM line; L: the query length (default: what the CIGAR consumes, or 30 for '*')."""
    if L is None:
        L, num = 0, ''
        for c in (cigar or ''):
            if c.isdigit():
                num += c
            else:
                L += int(num) if c in 'MIS=X' else 0
                num = ''
        L = L or 30
    cigar = '%dM' % L if cigar is None else cigar
    qual = C._qual(rng, L) if qual is None else qual
    return '\t'.join([name, str(flag), rname, str(pos), '60' if rname != '*' else '0', cigar, '*', '0', '0', C._seq(rng, L), qual, *tags])


def _sorted(lines, header):
    order = {ln.split('\t')[1][3:]: k for k, ln in enumerate(x for x in header if x.startswith('@SQ'))}
    order['*'] = 1 << 40
    return sorted(lines, key=lambda ln: (order[ln.split('\t')[2]], int(ln.split('\t')[3])))


def edges(rng):
    """Tens of records over HEADER: one per rule of the index (SAM positions are 1-based: pos = beg + 1)."""
    r = lambda *a, **k: record(rng, *a, **k)             # noqa: E731
    lines = [
        r('first', 'chr1', 1),                                            # [0, 30): bin 4681
        r('level4', 'chr1', 16380, '10M'),                                # crosses a 16 kb boundary
        r('three_windows', 'chr1', 16001, '5M33000N5M'),                  # windows 0, 1, 2 through an N
        r('level3', 'chr1', 131070, '10M'),                               # crosses a 128 kb boundary
        r('level0', 'chr1', (1 << 26) - 4, '10M'),                        # crosses a 2^26 boundary: bin 0
        r('no_cigar', 'chr1', 500000, '*'),                               # span 0
        r('all_insertion', 'chr1', 500000, '10I'),
        r('soft', 'chr1', 500010, '3S5M2D5M2S'),
        r('placed_unmapped', 'chr1', 500020, '*', flag=4),
        r('placed_unmapped_cigar', 'chr1', 500020, '30M', flag=4),        # flag 4: end = beg + 1 whatever the CIGAR says
        r('pos0', 'chr1', 0, '*', flag=4),                                # POS 0 with a reference: pos -1, beg 0
        r('far', 'chr1', 200000001, '5M3000000N5M'),
        r('chr2_a', 'chr2', 100),                                         # the reference changes in mid-slab; `empty` has none
        r('chr2_b', 'chr2', 100),
        r('chrM_in', 'chrM', 10),
        r('chrM_overhang', 'chrM', 16560, '5M40000N5M'),                  # beyond LN, beyond the reference's windows
        r('lost1', '*', 0, '*', flag=4),
        r('lost2', '*', 0, '*', flag=4, tags=('RG:Z:rg1',)),
        r('lost3', '*', 0, '*', flag=77, tags=('RG:Z:rg2',)),
    ]
    lines += [r('w%d' % k, 'chr1', 30000 + 40 * k) for k in range(20)]    # a run of one bin, then the next window
    return _sorted(lines, HEADER)


def many(rng, n=1500, lo=90, hi=150):
    """n records over three references (several BGZF blocks): runs of one bin, bins that come back, records over block cuts."""
    lines = []
    for k in range(n):
        L = int(rng.integers(lo, hi + 1))
        where = k * 3 // n
        lines.append(record(rng, 'm%d' % k, ('chr1', 'chr2', 'chrM')[where], 1 + (k * 7919) % (16000 if where == 2 else 400000), L=L,
                            flag=int(rng.choice([0, 16, 99, 147])), tags=('RG:Z:rg%d' % (k % 3), 'NM:i:%d' % (k % 7))))
    lines += [record(rng, 'x%d' % k, 'chr1', 16384 * k - 50, L=100) for k in (1, 2, 3)]     # over 16 kb cuts: bin 585 comes back
    lines += [record(rng, 'u%d' % k, '*', 0, '*', flag=4) for k in range(5)]
    return _sorted(lines, HEADER)


def block_end(rng):
    """Records of which one ends exactly where a BGZF block ends: a Z tag pads it until the stream up to it is 65280 bytes."""
    lines = [record(rng, 'b%d' % k, 'chr1', 100 + 50 * k, L=100) for k in range(400)]
    head = len(bamwriter.sam_to_bam_bytes(C.sam_text([], HEADER)))
    ends = np.cumsum([head] + [len(bamwriter.sam_to_bam_bytes(C.sam_text([ln], HEADER))) - head for ln in lines])
    size = lambda k: int(ends[k]) if 'XP:Z:' not in lines[k - 1] else len(bamwriter.sam_to_bam_bytes(C.sam_text(lines[:k], HEADER)))  # noqa: E731
    k = next(k for k in range(1, len(lines)) if size(k + 1) > BLOCK - 8) - 1                  # record k ends some way below the cut
    pad = BLOCK - size(k + 1) - 6                        # XP:Z: + NUL = 3 + pad + 1 bytes ... plus the pad itself
    assert pad >= 0
    lines[k] += '\tXP:Z:' + 'p' * (pad + 2)
    assert size(k + 1) == BLOCK, size(k + 1)
    return lines, k


def long_cigar(rng):
    """A record with 65535 CIGAR operations between two plain ones."""
    cigar = '1M1I' * 32767 + '1M'
    return [record(rng, 'before', 'chr1', 10), record(rng, 'ops65535', 'chr1', 20, cigar), record(rng, 'after', 'chr1', 40000)]


def big(rng):
    """Over BIG (an LN of 2^29 + 1: CSI, depth 6): records below and above 2^29, one ending at the reference's last base."""
    r = lambda *a, **k: record(rng, *a, **k)             # noqa: E731
    top = (1 << 29) + 1
    lines = [r('s1', 'small', 5), r('s2', 'small', 69990, '10M'),
             r('lowA', 'wheat3B', 1000), r('lowB', 'wheat3B', (1 << 26) - 4, '10M'), r('below', 'wheat3B', (1 << 29) - 4, '10M'),
             r('above', 'wheat3B', (1 << 29) + 1 - 9, '10M'), r('lost', '*', 0, '*', flag=4)]
    assert top - 9 + 10 - 1 == top                       # `above` ends at the last base
    return _sorted(lines, BIG)


def parsed(tmp_path, lines, header=HEADER, seed=5, name='in.sam'):
    """The lines as a parsed file with planes: dict(bam, seq, out, keep, pitch, text, path)."""
    from kbbq import aln
    path = tmp_path / name
    text = C.sam_text(lines, header)
    path.write_text(text)
    bam = aln.AlignmentFile(str(path))
    seq, out, keep, pitch = C.planes(bam, np.random.default_rng(seed))
    return dict(bam=bam, seq=seq, out=out, keep=keep, pitch=pitch, text=text, path=str(path))


def written(case, rows, index, deflate, set_oq=False, to_engine=lambda a: a):
    """(BAM bytes, the closed writer) of a parsed case through BamWriter in slabs of `rows` records; to_engine: where the planes
    have to lie (the GPU engine takes device tensors)."""
    from kbbq import _bamout
    bam, n = case['bam'], len(case['bam'])
    raw = io.BytesIO()
    with _bamout.BamWriter(raw, deflate=deflate, index=index) as w:
        w.header(bam)
        for first in range(0, n, rows):
            m = min(rows, n - first)
            w.records(bam.batch(), first, m, set_oq, case['keep'][first:first + m], to_engine(case['seq'][first:first + m]),
                      to_engine(case['out'][first:first + m]), case['pitch'])
    return raw.getvalue(), w
