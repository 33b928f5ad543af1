"""Test infrastructure of --bam-index: the executable model of the index (include/kbbq_hip.h "BAM index"), in plain Python and
independent of the product's code.  From the bytes of a BAM file -- every gzip member inflated on its own, its file offset kept --
the records are walked and the BAI (SAM specification 5.2) or CSI index is built rule by rule; parse() reads index bytes back,
query() is the specifications' reg2bins region query."""
import gzip
import struct
import zlib

BLOCK = 65280
MIN_SHIFT = 14
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def reg2bin(beg, end, min_shift=MIN_SHIFT, depth=5):
    """The smallest bin that holds [beg, end) (SAM specification 5.3; the CSI specification for other depths)."""
    end -= 1
    s, t = min_shift, ((1 << depth * 3) - 1) // 7
    level = depth
    while level > 0:
        if beg >> s == end >> s:
            return t + (beg >> s)
        level -= 1
        s += 3
        t -= 1 << level * 3
    return 0


def reg2bins(beg, end, min_shift=MIN_SHIFT, depth=5):
    """Every bin that may hold a record overlapping [beg, end)."""
    end -= 1
    bins = []
    s, t = min_shift + depth * 3, 0
    for level in range(depth + 1):
        bins.extend(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
        t += 1 << level * 3
    return bins


def depth_for(longest):
    depth = 5
    while 1 << (MIN_SHIFT + 3 * depth) < longest:
        depth += 1
    return depth


def pseudo_bin(fmt, depth):
    return 37450 if fmt == 'bai' else ((1 << (3 * depth + 3)) - 1) // 7 + 1


def members(data):
    """[(file offset, inflated bytes)] of the gzip members of a BGZF file, from BSIZE."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b'\x1f\x8b\x08\x04' and data[at + 12:at + 14] == b'BC', at
        size = struct.unpack_from('<H', data, at + 16)[0] + 1
        out.append((at, gzip.decompress(data[at:at + size])))
        at += size
    return out


class Bam:
    """A BAM file taken apart: refs [(name, LN)], records (dicts with ref, pos, flag, end, bin per depth on demand, start / stop as
    stream offsets), and the virtual offset of every stream offset."""

    def __init__(self, data):
        self.members = members(data)
        assert self.members and self.members[-1][1] == b'' and data.endswith(EOF)
        self.stream = b''.join(text for _, text in self.members)
        self.starts = []                                 # stream offset of every member's text
        at = 0
        for _, text in self.members:
            self.starts.append(at)
            at += len(text)
        s = self.stream
        assert s[:4] == b'BAM\1'
        l_text = struct.unpack_from('<i', s, 4)[0]
        at = 8 + l_text
        n_ref = struct.unpack_from('<i', s, at)[0]
        at += 4
        self.refs = []
        for _ in range(n_ref):
            l_name = struct.unpack_from('<i', s, at)[0]
            name = s[at + 4:at + 4 + l_name - 1].decode()
            self.refs.append((name, struct.unpack_from('<i', s, at + 4 + l_name)[0]))
            at += 8 + l_name
        self.records = []
        while at < len(s):
            size = struct.unpack_from('<i', s, at)[0]
            ref, pos, l_name, _, _, n_cigar, flag = struct.unpack_from('<iiBBHHH', s, at + 4)
            span = 0
            if not flag & 4:
                for k in range(n_cigar):
                    word = struct.unpack_from('<I', s, at + 36 + l_name + 4 * k)[0]
                    if word & 15 in (0, 2, 3, 7, 8):
                        span += word >> 4
            beg = max(pos, 0)
            self.records.append(dict(ref=ref, pos=pos, flag=flag, beg=beg, end=beg + max(span, 1), start=at, stop=at + 4 + size))
            at += 4 + size
        assert at == len(s)

    def voffset(self, u):
        """coff[u / 65280] << 16 | u % 65280, coff[b] the file offset of member b: the stream is cut every 65280 bytes, so behind
        the last byte of a full member this is the NEXT member's start (what htslib's bgzf_tell gives there) -- the EOF block's
        when the stream ends on a cut."""
        assert 0 <= u <= len(self.stream) and all(len(text) == BLOCK for _, text in self.members[:-2])
        k = u // BLOCK
        assert self.starts[k] == k * BLOCK and u - self.starts[k] <= len(self.members[k][1])
        return self.members[k][0] << 16 | u % BLOCK


def build(data, fmt='auto'):
    """(index bytes -- CSI: before compression --, format, depth) of the BAM file `data`."""
    bam = Bam(data)
    longest = max([ln for _, ln in bam.refs], default=0)
    if fmt == 'auto':
        fmt = 'bai' if longest <= 1 << 29 else 'csi'
    depth = 5 if fmt == 'bai' else depth_for(longest)
    assert fmt == 'csi' or longest <= 1 << 29
    v = {}                                               # memo of voffsets

    def vo(u):
        if u not in v:
            v[u] = bam.voffset(u)
        return v[u]
    n_ref = len(bam.refs)
    bins = [dict() for _ in range(n_ref)]                # bin -> [[beg, end]] chunks, one per run, in file order
    windows = [((max(ln, 1) + 16383) >> 14) + 1 for _, ln in bam.refs]
    linear = [[None] * w for w in windows]
    meta = [None] * n_ref                                # [ref_beg, ref_end, n_mapped, n_unmapped]
    n_no_coor = 0
    previous = None
    for r in bam.records:
        if r['ref'] < 0:
            n_no_coor += 1
            previous = None
            continue
        ref = r['ref']
        assert r['end'] <= 1 << (MIN_SHIFT + 3 * depth)
        b = reg2bin(r['beg'], r['end'], MIN_SHIFT, depth)
        chunk = [vo(r['start']), vo(r['stop'])]
        if previous == (ref, b):
            bins[ref][b][-1][1] = chunk[1]               # the run goes on
        else:
            bins[ref].setdefault(b, []).append(chunk)
        previous = (ref, b)
        for w in range(r['beg'] >> 14, ((r['end'] - 1) >> 14) + 1):
            w = min(w, windows[ref] - 1)
            if linear[ref][w] is None or chunk[0] < linear[ref][w]:
                linear[ref][w] = chunk[0]
        if meta[ref] is None:
            meta[ref] = [chunk[0], chunk[1], 0, 0]
        meta[ref][1] = chunk[1]
        meta[ref][3 if r['flag'] & 4 else 2] += 1
    out = [b'BAI\1' if fmt == 'bai' else b'CSI\1' + struct.pack('<iii', MIN_SHIFT, depth, 0), struct.pack('<i', n_ref)]
    for ref in range(n_ref):
        # neighbouring chunks of a bin whose end and begin lie in one compressed block are one chunk
        for b, chunks in bins[ref].items():
            merged = [chunks[0]]
            for c in chunks[1:]:
                if merged[-1][1] >> 16 >= c[0] >> 16:
                    merged[-1][1] = c[1]
                else:
                    merged.append(c)
            bins[ref][b] = merged
        filled = [w for w, x in enumerate(linear[ref]) if x is not None]
        n_intv = filled[-1] + 1 if filled else 0
        back = linear[ref][:n_intv]
        for w in range(n_intv - 2, -1, -1):
            if back[w] is None:
                back[w] = back[w + 1]
        out.append(struct.pack('<i', len(bins[ref]) + (meta[ref] is not None)))
        for b in sorted(bins[ref]):
            chunks = bins[ref][b]
            if fmt == 'bai':
                out.append(struct.pack('<Ii', b, len(chunks)))
            else:
                level, first = 0, 0
                while b >= first + (1 << 3 * level):
                    first += 1 << 3 * level
                    level += 1
                w = min((b - first) << 3 * (depth - level), windows[ref] - 1)
                out.append(struct.pack('<IQi', b, back[w] if w < n_intv else 0, len(chunks)))
            out.extend(struct.pack('<QQ', *c) for c in chunks)
        if meta[ref] is not None:
            out.append(struct.pack('<Ii', pseudo_bin(fmt, depth), 2) if fmt == 'bai' else struct.pack('<IQi', pseudo_bin(fmt, depth), 0, 2))
            out.append(struct.pack('<QQQQ', *meta[ref]))
        if fmt == 'bai':
            out.append(struct.pack('<i', n_intv))
            out.extend(struct.pack('<Q', x) for x in back)
    out.append(struct.pack('<Q', n_no_coor))
    return b''.join(out), fmt, depth


def inflate(data):
    """The text of a BGZF file (a CSI index is one)."""
    assert data.endswith(EOF)
    return b''.join(text for _, text in members(data))


def parse(data):
    """Index bytes (CSI: inflated) -> dict(fmt, depth, refs=[dict(bins={bin: chunks}, loffset={bin: v}, linear=[...], meta)],
    n_no_coor).  Every byte is accounted for."""
    fmt = {b'BAI\1': 'bai', b'CSI\1': 'csi'}[data[:4]]
    at, depth = 4, 5
    if fmt == 'csi':
        min_shift, depth, l_aux = struct.unpack_from('<iii', data, at)
        assert min_shift == MIN_SHIFT and l_aux == 0
        at += 12
    n_ref = struct.unpack_from('<i', data, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from('<i', data, at)[0]
        at += 4
        ref = dict(bins={}, loffset={}, linear=[], meta=None)
        for _ in range(n_bin):
            if fmt == 'bai':
                b, n_chunk = struct.unpack_from('<Ii', data, at)
                at += 8
            else:
                b, loffset, n_chunk = struct.unpack_from('<IQi', data, at)
                at += 16
                ref['loffset'][b] = loffset
            chunks = [struct.unpack_from('<QQ', data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == pseudo_bin(fmt, depth):
                assert n_chunk == 2
                ref['meta'] = chunks[0] + chunks[1]
                ref['loffset'].pop(b, None)
            else:
                assert b not in ref['bins'] and n_chunk > 0
                ref['bins'][b] = chunks
        if fmt == 'bai':
            n_intv = struct.unpack_from('<i', data, at)[0]
            ref['linear'] = list(struct.unpack_from('<%dQ' % n_intv, data, at + 4))
            at += 4 + 8 * n_intv
        refs.append(ref)
    n_no_coor = struct.unpack_from('<Q', data, at)[0]
    assert at + 8 == len(data)
    return dict(fmt=fmt, depth=depth, refs=refs, n_no_coor=n_no_coor)


def query(index, ref, beg, end):
    """The chunks a reader has to look at for [beg, end) of reference `ref`: those of the bins of reg2bins, without the ones
    that end at or before the linear index's (CSI: the bin's loffset) lower bound."""
    entry = index['refs'][ref]
    low = 0
    if index['fmt'] == 'bai' and entry['linear']:
        low = entry['linear'][min(beg >> 14, len(entry['linear']) - 1)]
    chunks = []
    for b in reg2bins(beg, end, MIN_SHIFT, index['depth']):
        for c in entry['bins'].get(b, ()):
            if c[1] > max(low, entry['loffset'].get(b, 0)):
                chunks.append(c)
    return sorted(chunks)


def record_at(bam, voffset):
    """The record of a Bam that starts at a virtual offset (None when none does)."""
    coff, within = voffset >> 16, voffset & 0xFFFF
    for k, (off, _) in enumerate(bam.members):
        if off == coff:
            u = bam.starts[k] + within
            return next((r for r in bam.records if r['start'] == u), None)
    return None


def crc_ok(data):
    """Every member's CRC32 and ISIZE are those of its text."""
    at = 0
    for off, text in members(data):
        size = struct.unpack_from('<H', data, off + 16)[0] + 1
        crc, isize = struct.unpack_from('<II', data, off + size - 8)
        if crc != zlib.crc32(text) & 0xFFFFFFFF or isize != len(text):
            return False
        at = off + size
    return at == len(data)
