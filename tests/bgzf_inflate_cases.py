"""BGZF members for the inflate kernel's tests (csrc/kbbq_bgzf_inflate.h): the valid ones and the fixed list of damaged ones.

Built once per process with Python's zlib, tests/bgzf_model.py (the project's own writer format) and by hand; shared by
test_bgzf_inflate_host.py (the host twin, no GPU) and test_gpu_bgzf_inflate.py (the kernel), so that the device only ever sees
damaged members the twin has already refused.  tests/tools/fuzz_bgzf_inflate.cpp builds the same list in C++ for the sanitizers.
"""
import functools
import struct
import zlib

import numpy as np

HEAD = bytes.fromhex('1f8b08040000000000ff060042430200')
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def frame(payload, text=None, isize=None, crc=None):
    """One BGZF member around a raw deflate payload; the trailer from `text`, or as given."""
    if text is not None:
        isize = len(text) if isize is None else isize
        crc = zlib.crc32(text) if crc is None else crc
    size = 18 + len(payload) + 8
    assert size <= 65536
    return HEAD + struct.pack('<H', size - 1) + bytes(payload) + struct.pack('<II', crc & 0xffffffff, isize & 0xffffffff)


def raw(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_at is None:
        return c.compress(text) + c.flush()
    return c.compress(text[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[flush_at:]) + c.flush()


def fastq_like(n, seed=5):
    """n bytes that look like FASTQ: names, bases, '+', qualities."""
    rng = np.random.default_rng(seed)
    out, k = [], 0
    while sum(map(len, out)) < n:
        seq = bytes(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), 100))
        qual = bytes((rng.integers(0, 8, 100) + 60).astype(np.uint8))
        out.append(b'@read%d/1\n%s\n+\n%s\n' % (k, seq, qual))
        k += 1
    return b''.join(out)[:n]


@functools.lru_cache(maxsize=None)
def valid():
    """[(name, text, payload)]: every kind of member RFC 1951 allows inside a BGZF block."""
    import bgzf_model as M
    rng = np.random.default_rng(9)
    text = fastq_like(20000)
    out = [('level %d' % lv, text, raw(text, lv)) for lv in (0, 1, 6, 9)]
    out.append(('Z_FIXED', text, raw(text, 6, zlib.Z_FIXED)))
    out.append(('full flush: several blocks and an empty stored one', text, raw(text, 6, flush_at=9000)))
    for n in (0, 1, 65280, 65536):
        t = fastq_like(n, seed=n + 1)
        out.append(('%d bytes' % n, t, raw(t, 6)))
    out.append(('65536 equal bytes: distance 1, length 258', b'A' * 65536, raw(b'A' * 65536, 9)))
    # zlib itself never looks back farther than 32768 - 262: the longest distance is written by hand, in the fixed code
    noise = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    b = Bits().put(1, 1).put(1, 2)
    for c in noise:
        b.ll(c)
    b.ll(285).code(29, 5).put(32768 - 24577, 13).ll(256)
    out.append(('a repeat at distance 32768', noise + noise[:258], b.bytes()))
    noise = rng.integers(0, 256, 50000, dtype=np.uint8).tobytes()
    out.append(('random bytes: zlib stores them', noise, raw(noise, 6)))
    out.append(('Huffman only', text[:3000], raw(text[:3000], 6, zlib.Z_HUFFMAN_ONLY)))
    out.append(('the empty member of the EOF block', b'', EOF[18:-8]))
    # literal codes of up to 15 bits (byte k 2^k times, no matches), distance codes of up to 15 bits (written by hand)
    skew = np.repeat(np.arange(15, dtype=np.uint8) + 65, 1 << np.arange(15))
    skew = rng.permutation(skew).tobytes()
    out.append(('literal codes of 15 bits', skew, raw(skew, 6, zlib.Z_HUFFMAN_ONLY)))
    out.append(('distance codes of 15 bits',) + long_distance_codes())
    # the project's own writer (bz_deflate, through its host model): the dynamic form and the stored form
    for name, t in (('own writer, dynamic', fastq_like(2500, seed=3)), ('own writer, stored', noise[:300])):
        packed, sizes, _ = M.deflate(t)
        assert len(sizes) == 1
        out.append((name, t, packed[18:-8]))
    for name, t, payload in out:
        assert zlib.decompress(payload, -15) == t, name
    assert out[-1][2][0] & 6 == 0 and out[-2][2][0] & 6 == 4               # stored, dynamic
    assert out[2][2][0] & 6 == 4 and out[4][2][0] & 6 == 2                 # level 6: dynamic; Z_FIXED: fixed
    return out


class Bits:
    """Hand-packed deflate bits."""

    def __init__(self):
        self.out, self.v, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        self.v |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        if self.n >= 64:
            whole = self.n >> 3
            self.out += (self.v & ((1 << (8 * whole)) - 1)).to_bytes(whole, 'little')
            self.v >>= 8 * whole
            self.n -= 8 * whole
        return self

    def code(self, c, nbits):                     # a Huffman code: its first bit first
        r = 0
        for i in range(nbits):
            r |= ((c >> i) & 1) << (nbits - 1 - i)
        return self.put(r, nbits)

    def ll(self, s):                              # the fixed literal/length code (RFC 1951 3.2.6)
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xc0 + s - 280, 8)

    def bytes(self):
        return bytes(self.out) + self.v.to_bytes((self.n + 7) // 8, 'little')


def long_distance_codes():
    """(text, payload): one dynamic block whose distance symbols 0..15 have codes of 1, 2, ..., 14, 15 and 15 bits -- a complete
    code far beyond the decoder's primary table -- each used once at its largest distance; the code-length code gives every length
    0..15 four bits."""
    import bgzf_model as M
    ll = [0] * 258
    ll[ord('a')] = ll[ord('b')] = ll[256] = ll[257] = 2
    d = list(range(1, 16)) + [15]
    b = Bits().put(1, 1).put(2, 2).put(258 - 257, 5).put(16 - 1, 5).put(19 - 4, 4)
    for s in M.CL_ORDER:
        b.put(0 if s >= 16 else 4, 3)
    for l in ll + d:
        b.code(l, 4)
    code_ll, code_d = M._canonical(ll), M._canonical(d)
    text = bytearray()
    for bit in np.random.default_rng(2).integers(0, 2, 256):
        s = ord('a') + int(bit)
        b.code(code_ll[s], 2)
        text.append(s)
    for ds in range(16):
        dist = M.DIST_HIGH[ds]
        b.code(code_ll[257], 2).code(code_d[ds], d[ds]).put(dist - M.DIST_BASE[ds], M.DIST_EXTRA[ds])
        for _ in range(3):
            text.append(text[-dist])
    b.code(code_ll[256], 2)
    return bytes(text), b.bytes()


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, payload, isize, crc)]: the fixed list.  Every one of them must get a status; none may be written outside its range."""
    name, text, payload = valid()[2]                                      # level 6: one dynamic block
    crc, n = zlib.crc32(text), len(text)
    out = [('truncated in the block header', b'', n, crc), ('truncated in the code lengths', payload[:10], n, crc),
           ('truncated in the body', payload[:len(payload) // 2], n, crc), ('truncated before the end', payload[:-1], n, crc)]
    flipped = bytearray(payload)
    flipped[len(payload) // 2] ^= 0x10
    out.append(('a flipped payload bit', bytes(flipped), n, crc))
    out.append(('a flipped CRC bit', payload, n, crc ^ 0x100))
    out.append(('a flipped ISIZE bit', payload, n ^ 4, crc))
    out.append(('an ISIZE smaller than the output', payload, n - 100, crc))
    hand = lambda nm, b: out.append((nm, b.bytes(), 4, 0))               # noqa: E731
    hand('a distance before the start', Bits().put(1, 1).put(1, 2).ll(ord('a')).ll(257).code(1, 5).ll(256))
    for s in (286, 287):
        hand('literal/length symbol %d' % s, Bits().put(1, 1).put(1, 2).ll(ord('a')).ll(s).code(0, 5).ll(256))
    for s in (30, 31):
        hand('distance symbol %d' % s, Bits().put(1, 1).put(1, 2).ll(ord('a')).ll(257).code(s, 5).ll(256))
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    hand('an over-subscribed code', b.put(0, 32))
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4).put(1, 3)
    for _ in range(18):
        b.put(0, 3)
    hand('an incomplete code', b.put(0, 32))
    hand('block type 3', Bits().put(1, 1).put(3, 2).put(0, 29))
    hand('stored LEN / NLEN', Bits().put(1, 1).put(0, 2).put(0, 5).put(4, 16).put(0xfffa, 16).put(0x64636261, 32))
    return out


def zlib_says(payload, isize, crc):
    """The text, if zlib inflates the payload to exactly isize bytes with that CRC32; else None."""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(bytes(payload))
    except zlib.error:
        return None
    if not d.eof or len(text) != isize or zlib.crc32(text) != crc:
        return None
    return text
