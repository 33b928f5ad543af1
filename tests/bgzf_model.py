"""Host model of the BGZF deflate kernel (csrc/kbbq_bgzf.h) and a decoder that lists the tokens of a block it wrote.

tokens(payload)        a recording inflater for raw DEFLATE (RFC 1951): per block the BTYPE, the three lists of code lengths and
                       every token with its bit offset and size; and the inflated text.
deflate_block(text)    the BGZF member bz_deflate is specified to write for one block, as plain sequential code after the header
                       comment of kbbq_bgzf.h, and a record of the paths the block took.
deflate(text, bb)      the members of all blocks joined, their sizes and records.  `grid` workgroups share the blocks as the
                       kernel's do (b, b + grid, ...), each through one State, so that what must be reset between two blocks of a
                       workgroup can be stated -- and, with broken=, left out.
verify(text, bb, packed, sizes)   what every test asks of blocks somebody wrote, the GPU or this model.

Plain Python and NumPy; zlib is used as the judge in verify() and for the CRC of a strip only."""
import bisect
import gzip
import heapq
import struct
import zlib

import numpy as np

TILE, HASH_BITS = 512, 14
MIN_MATCH, MAX_MATCH, MAX_DIST, BLOCK_MAX = 4, 258, 32768, 65280
THREADS = 512
HEAD = bytes.fromhex('1f8b08040000000000ff060042430200')
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
BROKEN = ('third_word', 'stale_lengths', 'no_repair_7', 'crc_shift')

# RFC 1951, 3.2.5
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
DIST_BASE = [1]
for _e in DIST_EXTRA[:-1]:
    DIST_BASE.append(DIST_BASE[-1] + (1 << _e))
assert len(LEN_BASE) == 29 and len(DIST_BASE) == 30 and DIST_BASE[-1] + (1 << 13) - 1 == 32768
DIST_LOW = list(DIST_BASE)
DIST_HIGH = [b + (1 << e) - 1 for b, e in zip(DIST_BASE, DIST_EXTRA)]

_LEN_SYM = np.zeros(259, dtype=np.int64)
for _i, (_b, _e) in enumerate(zip(LEN_BASE, LEN_EXTRA)):
    _LEN_SYM[_b:_b + (1 << _e)] = 257 + _i                 # 258 is written twice: symbol 285, no extra bits, has the last word
_LEN_BASE = np.array(LEN_BASE, dtype=np.int64)
_LEN_EXTRA = np.array(LEN_EXTRA, dtype=np.int64)
_DIST_BASE = np.array(DIST_BASE, dtype=np.int64)
_DIST_EXTRA = np.array(DIST_EXTRA, dtype=np.int64)


def dist_sym(d):
    return np.searchsorted(_DIST_BASE, d, side='right') - 1


# ---- the recording inflater ----------------------------------------------------------------------------------------------
class _Reader:
    def __init__(self, data):
        self.data, self.at, self.bits = bytes(data) + bytes(8), 0, 8 * len(data)

    def peek(self, n):                                     # n <= 57
        return (int.from_bytes(self.data[self.at >> 3:(self.at >> 3) + 8], 'little') >> (self.at & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.at += n
        if self.at > self.bits:
            raise ValueError('deflate stream ends inside a code')
        return v


def _canonical(lens):
    """{symbol: (code, sent first bit first)} of a list of code lengths (RFC 1951, 3.2.2)."""
    top = max(lens) if lens else 0
    count = [0] * (top + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, first = 0, [0] * (top + 2)
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        first[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = first[l]
            first[l] += 1
    return out


def _reverse(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


class _Decoder:
    """Table decoder of one prefix code.  An over-subscribed list of lengths is refused; an incomplete one is allowed only in
    the form RFC 1951 allows, a single code of one bit."""

    def __init__(self, lens):
        used = [l for l in lens if l]
        self.top = max(used) if used else 0
        kraft = sum(1 << (self.top - l) for l in used)
        if used and kraft > (1 << self.top):
            raise ValueError('over-subscribed code')
        if used and kraft < (1 << self.top) and not (len(used) == 1 and used[0] == 1):
            raise ValueError('incomplete code')
        self.table = [None] * (1 << self.top)
        for s, c in _canonical(lens).items():
            l = lens[s]
            r = _reverse(c, l)
            self.table[r::1 << l] = [(s, l)] * (1 << (self.top - l))

    def read(self, rd):
        if not self.top:
            raise ValueError('a symbol of an empty code')
        e = self.table[rd.peek(self.top)]
        if e is None:
            raise ValueError('a code that no symbol has')
        rd.take(e[1])
        return e[0]


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_D = [5] * 32                                     # 30 and 31 have codes and never occur


def tokens(payload):
    """(blocks, text) of a raw DEFLATE stream.  A block is a dict: btype, final, ll / d / cl (lists of code lengths; fixed codes for
    BTYPE 1, empty for BTYPE 0), tokens [(bit offset, bits, literal byte | (length, distance))], eob (bit offset of the end-of-block
    code; for a stored block the offset after its last byte, with `stored` bytes), first (offset in the text of the block's first byte) and, for a
    dynamic block, header_bits.  `bits` counts a token's codes and extra bits.  `end` of the last block is where the stream ends."""
    rd = _Reader(payload)
    out = bytearray()
    blocks = []
    while True:
        final, btype = rd.take(1), rd.take(2)
        blk = dict(btype=btype, final=final, ll=[], d=[], cl=[], tokens=[], first=len(out))
        if btype == 0:
            rd.at = (rd.at + 7) & ~7
            n, nn = rd.take(16), rd.take(16)
            if n ^ nn != 0xffff:
                raise ValueError('stored block: LEN and NLEN disagree')
            if rd.at + 8 * n > rd.bits:
                raise ValueError('stored block longer than the stream')
            out += rd.data[rd.at >> 3:(rd.at >> 3) + n]
            rd.at += 8 * n
            blk['eob'], blk['stored'] = rd.at, n
        elif btype in (1, 2):
            if btype == 1:
                ll, d = _FIXED_LL, _FIXED_D
            else:
                start = rd.at - 3
                hlit, hdist, hclen = rd.take(5) + 257, rd.take(5) + 1, rd.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = rd.take(3)
                dec = _Decoder(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = dec.read(rd)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise ValueError('repeat with nothing before it')
                        lens += [lens[-1]] * (3 + rd.take(2))
                    else:
                        lens += [0] * ((3 + rd.take(3)) if s == 17 else (11 + rd.take(7)))
                if len(lens) != hlit + hdist:
                    raise ValueError('a run past the end of the code lengths')
                ll, d = lens[:hlit], lens[hlit:]
                blk['cl'] = cl
                blk['header_bits'] = rd.at - start
            blk['ll'], blk['d'] = list(ll), list(d)
            dec_ll = _Decoder(ll)
            dec_d = _Decoder(d) if any(d) else None
            toks = blk['tokens']
            while True:
                at = rd.at
                s = dec_ll.read(rd)
                if s < 256:
                    out.append(s)
                    toks.append((at, rd.at - at, s))
                elif s == 256:
                    blk['eob'] = at
                    break
                else:
                    if s > 285 or dec_d is None:
                        raise ValueError('a length with no distance code')
                    length = LEN_BASE[s - 257] + rd.take(LEN_EXTRA[s - 257])
                    ds = dec_d.read(rd)
                    if ds > 29:
                        raise ValueError('distance symbol %d' % ds)
                    dist = DIST_BASE[ds] + rd.take(DIST_EXTRA[ds])
                    if dist > len(out):
                        raise ValueError('a distance before the first byte')
                    for _ in range(length):
                        out.append(out[-dist])
                    toks.append((at, rd.at - at, (length, dist)))
        else:
            raise ValueError('BTYPE 3')
        blk['end'] = rd.at
        blocks.append(blk)
        if final:
            return blocks, bytes(out)


def unlimited_depth(freq):
    """Depth of a Huffman tree over the non-zero counts, built with a heap and no limit (the least deep of the equal-cost
    trees: ties go to the shallower subtree)."""
    heap = [(f, 0) for f in freq if f]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def paths(blk):
    """What a decoded block (tokens()) shows of the paths its encoder took: the symbols' counts, the largest token, whether a
    token needed the third word of bz_put (the payload starts at bit 16 of the kernel's word buffer), lengths, distances, and
    the largest number of bytes a match carried into the next 512-byte tile."""
    freq_ll, freq_d = [0] * 286, [0] * 30
    freq_ll[256] = 1
    rec = dict(max_token_bits=0, three_words=0, lengths=set(), dists=set(), pairs=set(), max_carry=0, starts_511=set(),
               freq_ll=freq_ll, freq_d=freq_d)
    p = 0
    for at, bits, t in blk['tokens']:
        rec['max_token_bits'] = max(rec['max_token_bits'], bits)
        if ((16 + at) & 31) + bits > 64:
            rec['three_words'] += 1
        if isinstance(t, tuple):
            length, dist = t
            freq_ll[int(_LEN_SYM[length])] += 1
            freq_d[int(dist_sym(dist))] += 1
            rec['lengths'].add(length)
            rec['dists'].add(dist)
            rec['pairs'].add(t)
            if p // TILE != (p + length) // TILE:
                rec['max_carry'] = max(rec['max_carry'], (p + length) % TILE)
            if p % TILE == TILE - 1:
                rec['starts_511'].add(length)
            p += length
        else:
            freq_ll[t] += 1
            p += 1
    return rec


def cl_freq(blk):
    """Counts of the code-length symbols a dynamic block's header holds, found by coding its lengths again as the header comment
    says (16 / 17 / 18 in that order) -- asserted equal in number of bits to the header read."""
    stream = _cl_stream(blk['ll'] + blk['d'])
    freq = [0] * 19
    for s, _ in stream:
        freq[s] += 1
    bits = 17 + 3 * (max(i for i in range(19) if blk['cl'][CL_ORDER[i]] or i < 4) + 1)
    bits += sum(blk['cl'][s] + (2 if s == 16 else 3 if s == 17 else 7 if s == 18 else 0) for s, _ in stream)
    assert bits == blk['header_bits'], (bits, blk['header_bits'])
    return freq


# ---- the encoder ---------------------------------------------------------------------------------------------------------
def _cl_stream(lens):
    out, i, n = [], 0, len(lens)
    while i < n:
        v, run = lens[i], 1
        while i + run < n and lens[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 3:
                r = min(run, 138)
                out.append((18, r - 11) if r >= 11 else (17, r - 3))
                run -= r
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
    return out


def build_code(freq, limit, length, code, repair=True):
    """bz_rank and bz_build_code: lengths of at most `limit` bits into length[], canonical codes (bit-reversed) into code[], for
    the symbols with a count.  Entries of the others are left as they are.  Returns the depth before limiting."""
    order = sorted((f, s) for s, f in enumerate(freq) if f)  # ascending (count, symbol)
    m = len(order)
    if m == 0:
        return 0
    A, sym = [f for f, _ in order], [s for _, s in order]
    if m == 1:
        A[0] = 1
    else:
        A[0] += A[1]
        root, leaf = 0, 2
        for nx in range(1, m - 1):
            if leaf >= m or A[root] < A[leaf]:
                A[nx] = A[root]
                A[root] = nx
                root += 1
            else:
                A[nx] = A[leaf]
                leaf += 1
            if leaf >= m or (root < nx and A[root] < A[leaf]):
                A[nx] += A[root]
                A[root] = nx
                root += 1
            else:
                A[nx] += A[leaf]
                leaf += 1
        A[m - 2] = 0
        for nx in range(m - 3, -1, -1):
            A[nx] = A[A[nx]] + 1
        avbl, used, depth, root, nx = 1, 0, 0, m - 2, m - 1
        while avbl > 0:
            while root >= 0 and A[root] == depth:
                used += 1
                root -= 1
            while avbl > used:
                A[nx] = depth
                nx -= 1
                avbl -= 1
            avbl, depth, used = 2 * used, depth + 1, 0
    deepest = max(A)
    count = [0] * 17
    for a in A:
        count[min(a, limit)] += 1
    if m > 1 and repair:
        total = sum(count[i] << (limit - i) for i in range(1, limit + 1))
        while total != 1 << limit:
            count[limit] -= 1
            for i in range(limit - 1, 0, -1):
                if count[i]:
                    count[i] -= 1
                    count[i + 1] += 2
                    break
            total -= 1
    j = m
    for i in range(1, limit + 1):
        for _ in range(count[i]):
            j -= 1
            length[sym[j]] = i
    # canonical codes over every entry of length[] that is not zero, as the kernel's loop over the whole alphabet does
    nxt, c = [0] * 17, 0
    for bits in range(1, limit + 1):
        c = (c + (count[bits - 1] if bits > 1 else 0)) << 1
        nxt[bits] = c
    for s, l in enumerate(length):
        if l:
            code[s] = _reverse(nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return deepest


X2N = [0x40000000]


def _gf2_mul(a, b):
    """a * b mod P over GF(2), reflected, on uint32 arrays"""
    a, b = np.asarray(a, dtype=np.uint32), np.array(b, dtype=np.uint32)
    p = np.zeros(np.broadcast(a, b).shape, dtype=np.uint32)
    b = np.broadcast_to(b, p.shape).copy()
    for i in range(32):
        p ^= np.where(a & np.uint32(0x80000000 >> i), b, np.uint32(0))
        b = np.where(b & np.uint32(1), (b >> np.uint32(1)) ^ np.uint32(0xedb88320), b >> np.uint32(1))
    return p


while len(X2N) < 32:
    X2N.append(int(_gf2_mul(X2N[-1], X2N[-1])))


def _x8n(nbytes):
    nbytes = np.array(nbytes, dtype=np.int64)
    p = np.full(nbytes.shape, 0x80000000, dtype=np.uint32)
    k = 3
    while nbytes.any():
        p = np.where(nbytes & 1, _gf2_mul(np.uint32(X2N[k & 31]), p), p)
        nbytes >>= 1
        k += 1
    return p


def strip_length(n):
    L = ((n + THREADS - 1) // THREADS + 3) & ~3
    return L if L & 4 else L + 4


_X8N = {}


def _x8n_kept(nbytes):
    """_x8n, every power worked out once: the blocks of one launch ask for the same ones again and again"""
    miss = sorted(set(nbytes) - _X8N.keys())
    if miss:
        _X8N.update(zip(miss, _x8n(miss).tolist()))
    return np.array([_X8N[v] for v in nbytes], dtype=np.uint32)


def crc32_strips(text, off_by=0):
    """CRC32 the kernel's way: a strip a thread, each strip's CRC moved behind the bytes after it and xored in."""
    n = len(text)
    L = strip_length(n)
    lo = np.minimum(n, np.arange(THREADS, dtype=np.int64) * L)
    hi = np.minimum(n, lo + L)
    live = lo < hi
    lo, hi = lo[live], hi[live]
    if not len(lo):
        return 0
    c = np.array([zlib.crc32(text[a:b]) for a, b in zip(lo.tolist(), hi.tolist())], dtype=np.uint32)
    x = _x8n_kept((n - hi + off_by).tolist())
    return int(np.bitwise_xor.reduce(np.where(hi < n, _gf2_mul(x, c), c)))


def lz_parse(text):
    """The kernel's parse: (positions, lengths, distances) of the matches in text order, and the largest carry into a next
    tile.  Every position no match covers is a literal."""
    n = len(text)
    s = np.frombuffer(text, dtype=np.uint8)
    if n < MIN_MATCH + 1:
        return [], [], [], 0
    w = s.astype(np.uint32)
    v = w[:n - 3] | (w[1:n - 2] << np.uint32(8)) | (w[2:n - 1] << np.uint32(16)) | (w[3:] << np.uint32(24))
    h = ((v.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - HASH_BITS)
    h = h.astype(np.int64)
    cand = np.full(n, -1, dtype=np.int64)
    tab = np.full(1 << HASH_BITS, -1, dtype=np.int64)       # the latest position of the tiles before
    for t0 in range(0, n - 3, TILE):
        hi = min(t0 + TILE, n - 3)
        cand[t0:hi] = tab[h[t0:hi]]
        tab[h[t0:hi]] = np.arange(t0, hi)                   # ascending: of equal hashes the last one stays
    p = np.arange(n - 3)
    c = cand[:n - 3]
    ok = (c >= 0) & (p - c <= MAX_DIST)
    ok[ok] = v[c[ok]] == v[p[ok]]
    where = np.nonzero(ok)[0].tolist()
    pos, lens, dists, carry = [], [], [], 0
    at = 0
    while True:
        i = bisect.bisect_left(where, at)
        if i == len(where):
            break
        at = where[i]
        src = int(cand[at])
        most = min(MAX_MATCH, n - at)
        a, b = text[src:src + most], text[at:at + most]
        if a == b:
            l = most
        else:
            x = int.from_bytes(a, 'little') ^ int.from_bytes(b, 'little')
            l = ((x & -x).bit_length() - 1) >> 3
        pos.append(at)
        lens.append(l)
        dists.append(at - src)
        if at // TILE != (at + l) // TILE:
            carry = max(carry, (at + l) % TILE)
        at += l
    return pos, lens, dists, carry


class State:
    """What a workgroup keeps in LDS from block to block, as far as a block's bytes could depend on it."""

    def __init__(self):
        self.len_ll, self.len_d = [0] * 286, [0] * 30
        self.code_ll, self.code_d = [0] * 286, [0] * 30


def _pack(vals, nbits):
    vals = np.asarray(vals, dtype=np.uint64)
    nbits = np.asarray(nbits, dtype=np.int64)
    lane = np.arange(48, dtype=np.uint64)
    bits = ((vals[:, None] >> lane[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits[lane[None, :].astype(np.int64) < nbits[:, None]], bitorder='little').tobytes()


def deflate_block(text, state=None, broken=None):
    """(the BGZF member of one block, the record of its paths)."""
    assert broken is None or broken in BROKEN
    text = bytes(text)
    n = len(text)
    assert 1 <= n <= BLOCK_MAX
    st = state if state is not None else State()
    if broken != 'stale_lengths':
        st.len_ll, st.len_d, st.code_ll, st.code_d = [0] * 286, [0] * 30, [0] * 286, [0] * 30
    crc = crc32_strips(text, 1 if broken == 'crc_shift' else 0)

    pos, lens, dists, carry = lz_parse(text)
    s = np.frombuffer(text, dtype=np.uint8)
    covered = np.zeros(n + 1, dtype=np.int64)
    np.add.at(covered, pos, 1)
    np.add.at(covered, [p + l for p, l in zip(pos, lens)], -1)
    lit_pos = np.nonzero(np.cumsum(covered[:n]) == 0)[0]
    m_pos, m_len, m_dist = (np.array(x, dtype=np.int64) for x in (pos, lens, dists))
    ls = _LEN_SYM[m_len]
    ds = dist_sym(m_dist)
    freq_ll = np.bincount(np.concatenate([s[lit_pos].astype(np.int64), ls, [256]]), minlength=286).tolist()
    freq_d = np.bincount(ds, minlength=30).tolist()

    deep_ll = build_code(freq_ll, 15, st.len_ll, st.code_ll)
    deep_d = build_code(freq_d, 15, st.len_d, st.code_d)

    # bz_plan_header
    hlit, hdist = 286, 30
    while hlit > 257 and not st.len_ll[hlit - 1]:
        hlit -= 1
    while hdist > 1 and not st.len_d[hdist - 1]:
        hdist -= 1
    stream = _cl_stream(st.len_ll[:hlit] + st.len_d[:hdist])
    freq_cl = [0] * 19
    for sy, _ in stream:
        freq_cl[sy] += 1
    len_cl, code_cl = [0] * 19, [0] * 19
    deep_cl = build_code(freq_cl, 7, len_cl, code_cl, repair=broken != 'no_repair_7')
    used = [i for i in range(19) if len_cl[i]]
    lone = len(used) == 1
    if lone:
        only = used[0]
        other = 0 if only else 18
        len_cl[other] = 1
        code_cl[only], code_cl[other] = (0, 1) if only < other else (1, 0)
    hclen = 4
    for i in range(19):
        if len_cl[CL_ORDER[i]] and i + 1 > hclen:
            hclen = i + 1
    cl_extra = {16: 2, 17: 3, 18: 7}
    hdr = 17 + 3 * hclen + sum(len_cl[sy] + cl_extra.get(sy, 0) for sy, _ in stream)
    ll_extra = [0] * 257 + LEN_EXTRA
    body = sum(freq_ll[i] * (st.len_ll[i] + ll_extra[i]) for i in range(286))
    body += sum(freq_d[i] * (st.len_d[i] + DIST_EXTRA[i]) for i in range(30))
    coded = ((hdr + body + 7) >> 3) < n + 5

    # the tokens' bits, whether or not the block is sent coded: the record speaks of the coded form
    len_ll, code_ll = np.array(st.len_ll, dtype=np.int64), np.array(st.code_ll, dtype=np.uint64)
    len_d, code_d = np.array(st.len_d, dtype=np.int64), np.array(st.code_d, dtype=np.uint64)
    t_pos = np.concatenate([lit_pos, m_pos])
    lit = s[lit_pos].astype(np.int64)
    le, de = _LEN_EXTRA[ls - 257], _DIST_EXTRA[ds]
    lv, dv = (m_len - _LEN_BASE[ls - 257]).astype(np.uint64), (m_dist - _DIST_BASE[ds]).astype(np.uint64)
    n1 = len_ll[ls]
    n2 = n1 + le
    n3 = n2 + len_d[ds]
    m_val = code_ll[ls] | (lv << n1.astype(np.uint64)) | (code_d[ds] << n2.astype(np.uint64)) | (dv << n3.astype(np.uint64))
    t_val = np.concatenate([code_ll[lit], m_val])
    t_bits = np.concatenate([len_ll[lit], n3 + de])
    order = np.argsort(t_pos, kind='stable')
    t_val, t_bits = t_val[order], t_bits[order]
    t_at = hdr + np.cumsum(t_bits) - t_bits                 # bit offsets in the payload
    sh = (16 + t_at) & 31
    three = sh + t_bits > 64
    if broken == 'third_word' and three.any():
        keep = np.where(three, (np.uint64(1) << (64 - sh).astype(np.uint64)) - np.uint64(1), np.uint64(0xffffffffffffffff))
        t_val = t_val & keep

    rec = dict(n=n, coded=bool(coded), btype=2 if coded else 0, ntok=int(len(t_bits)), lone_cl=lone,
               limited=dict(ll=deep_ll > 15, d=deep_d > 15, cl=deep_cl > 7), depth=dict(ll=deep_ll, d=deep_d, cl=deep_cl),
               max_token_bits=int(t_bits.max()), three_words=int(three.sum()), long_tokens=int((t_bits >= 34).sum()),
               lengths=set(lens), dists=set(dists), pairs=set(zip(lens, dists)), max_carry=carry,
               header_bits=hdr, body_bits=body)

    if coded:
        h_val, h_bits = [5, hlit - 257, hdist - 1, hclen - 4], [3, 5, 5, 4]
        for i in range(hclen):
            h_val.append(len_cl[CL_ORDER[i]])
            h_bits.append(3)
        for sy, extra in stream:
            h_val.append(code_cl[sy] | (extra << len_cl[sy]))
            h_bits.append(len_cl[sy] + cl_extra.get(sy, 0))
        assert sum(h_bits) == hdr
        vals = np.concatenate([np.array(h_val, dtype=np.uint64), t_val, np.array([st.code_ll[256]], dtype=np.uint64)])
        nbits = np.concatenate([np.array(h_bits, dtype=np.int64), t_bits, [st.len_ll[256]]])
        payload = _pack(vals, nbits)
        assert len(payload) == (hdr + body + 7) >> 3 or broken
        payload = payload.ljust((hdr + body + 7) >> 3, b'\0')[:(hdr + body + 7) >> 3]
    else:
        payload = b'\x01' + struct.pack('<HH', n, n ^ 0xffff) + text
    size = 18 + len(payload) + 8
    return HEAD + struct.pack('<H', size - 1) + payload + struct.pack('<II', crc, n), rec


def deflate(text, block_bytes=BLOCK_MAX, grid=256, broken=None):
    """(packed members, sizes, records) of every block of `text`, `grid` workgroups walking the blocks as bz_deflate does."""
    text = bytes(text)
    nb = (len(text) + block_bytes - 1) // block_bytes
    members, recs = [None] * nb, [None] * nb
    for wg in range(min(grid, nb)):
        st = State()
        for b in range(wg, nb, grid):
            members[b], recs[b] = deflate_block(text[b * block_bytes:(b + 1) * block_bytes], st, broken)
    return b''.join(members), np.array([len(m) for m in members], dtype=np.int64), recs


# ---- the checker ---------------------------------------------------------------------------------------------------------
def verify(text, block_bytes, packed, sizes):
    """Every block of `packed`: header bytes, BSIZE, BFINAL, the bound; zlib inflates it alone to its piece and stops at its end;
    CRC32 and ISIZE are zlib's; tokens() reads the same text; every match is 4..258 bytes at 1..32768 and its source begins in
    an earlier 512-byte tile of the block than the match.  And gzip reads the whole.  Returns the decoded blocks."""
    text, packed = bytes(text), bytes(packed)
    sizes = [int(x) for x in sizes]
    nb = (len(text) + block_bytes - 1) // block_bytes
    assert len(sizes) == nb and sum(sizes) == len(packed)
    assert gzip.decompress(packed) == text
    out, at = [], 0
    for b, size in enumerate(sizes):
        piece = text[b * block_bytes:(b + 1) * block_bytes]
        blk = packed[at:at + size]
        at += size
        assert blk[:16] == HEAD and struct.unpack_from('<H', blk, 16)[0] == size - 1, b
        assert 26 < size <= len(piece) + 31, b
        payload = blk[18:-8]
        assert payload[0] & 1, b                            # BFINAL
        z = zlib.decompressobj(-15)
        assert z.decompress(payload) == piece and z.eof and z.unused_data == b'', b
        assert struct.unpack_from('<II', blk, size - 8) == (zlib.crc32(piece), len(piece)), b
        blocks, got = tokens(payload)
        assert got == piece and len(blocks) == 1, b
        d = blocks[0]
        assert (d['end'] + 7) >> 3 == len(payload), b       # nothing behind the end-of-block code but the padding of its byte
        p = 0
        for _, _, t in d['tokens']:
            if isinstance(t, tuple):
                length, dist = t
                assert MIN_MATCH <= length <= MAX_MATCH and 1 <= dist <= MAX_DIST and dist <= p, (b, p, t)
                assert (p - dist) // TILE < p // TILE, (b, p, t)
                p += length
            else:
                p += 1
        assert p == len(piece) or d['btype'] == 0, b
        out.append(d)
    assert at == len(packed)
    return out
