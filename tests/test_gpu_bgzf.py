"""kbbq_bgzf_deflate_dev / kbbq_bgzf_deflate on the MI355X (csrc/kbbq_bgzf.h), with zlib as the oracle: a block is right when
zlib.decompress(payload, -15) returns its text, and gzip.decompress of the packed blocks returns the whole text (which also
verifies every CRC32 and ISIZE).  The deflate headers are read here too (code lengths, used symbols), so that what a case is
about -- a code of two symbols with no distance code, lengths that needed limiting -- is seen in the block and not assumed."""
import ctypes
import gzip
import struct
import zlib

import numpy as np
import pytest

import kmer_model as M

pytestmark = pytest.mark.gpu

BLOCK = 65280
HEAD = bytes.fromhex('1f8b08040000000000ff060042430200')


def deflate(text, block_bytes=BLOCK, host=False):
    """(packed blocks, sizes, the blocks as written before packing) of `text` through the device call, or -- host=True -- the
    packed blocks through the host-buffer call."""
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    lib, ctx = N.load(), dev.context()
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    n = text.size
    bound = int(lib.kbbq_bgzf_bound(n, block_bytes))
    total = ctypes.c_size_t(0)
    if host:
        out = np.full(bound + 16, 0xAA, dtype=np.uint8)
        N.check(lib.kbbq_bgzf_deflate(ctx.handle, N.ptr(text), n, block_bytes, N.ptr(out), bound, ctypes.byref(total)))
        assert np.all(out[total.value:] == 0xAA)
        return out[:total.value].tobytes()
    nb = (n + block_bytes - 1) // block_bytes
    d_text = torch.from_numpy(text.copy()).cuda()
    d_blocks = torch.full((nb * N.BGZF_SLOT,), 0xAA, dtype=torch.uint8, device='cuda')
    d_sizes = torch.zeros(nb, dtype=torch.int32, device='cuda')
    d_packed = torch.full((bound + 16,), 0xAA, dtype=torch.uint8, device='cuda')
    N.check(lib.kbbq_bgzf_deflate_dev(ctx.handle, N.ptr(d_text), n, block_bytes, N.ptr(d_blocks), N.ptr(d_sizes), N.ptr(d_packed),
                                      ctypes.byref(total)))
    packed = d_packed.cpu().numpy()
    assert np.all(packed[total.value:] == 0xAA)                      # nothing past the packed length
    sizes = d_sizes.cpu().numpy().astype(np.int64)
    assert int(sizes.sum()) == total.value <= bound
    slots = d_blocks.cpu().numpy().reshape(nb, N.BGZF_SLOT)
    packed = packed[:total.value].tobytes()
    assert packed == b''.join(slots[b, :sizes[b]].tobytes() for b in range(nb))
    for b in range(nb):
        assert np.all(slots[b, (sizes[b] + 3) // 4 * 4:] == 0xAA)    # a block stays inside its slot: whole words, no more
    return packed, sizes, slots


def check(text, block_bytes=BLOCK):
    """Every block of `text`: header, BSIZE, the bound, inflates alone to its piece, CRC32, ISIZE.  Returns [(btype, size)]."""
    text = bytes(text)
    packed, sizes, _ = deflate(text, block_bytes)
    assert gzip.decompress(packed) == text
    out, at = [], 0
    for b, size in enumerate(sizes.tolist()):
        piece = text[b * block_bytes:(b + 1) * block_bytes]
        blk = packed[at:at + size]
        assert blk[:16] == HEAD and struct.unpack_from('<H', blk, 16)[0] == size - 1
        assert size <= len(piece) + 31
        z = zlib.decompressobj(-15)
        assert z.decompress(blk[18:-8]) == piece and z.eof and z.unused_data == b''
        assert struct.unpack_from('<II', blk, size - 8) == (zlib.crc32(piece), len(piece))
        out.append(((blk[18] >> 1) & 3, size))
        assert blk[18] & 1                                           # BFINAL
        at += size
    assert at == len(packed)
    return out


class Bits:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.at >> 3] >> (self.at & 7)) & 1) << i
            self.at += 1
        return v


def dynamic_header(payload):
    """(literal/length code lengths, distance code lengths, code-length code lengths) of a BTYPE 10 payload (RFC 1951, 3.2.7)."""
    bits = Bits(payload)
    assert bits.take(1) == 1 and bits.take(2) == 2
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = bits.take(3)
    code, codes = 0, {}
    for length in range(1, 8):                                       # canonical codes of the code-length code
        for s in range(19):
            if cl[s] == length:
                codes[length, code] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        v, length = 0, 0
        while (length, v) not in codes:
            v = (v << 1) | bits.take(1)
            length += 1
            assert length <= 7
        s = codes[length, v]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits.take(2))
        else:
            lens += [0] * ((3 + bits.take(3)) if s == 17 else (11 + bits.take(7)))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:], cl


def payload_of(packed, size=None):
    return packed[18:(size or len(packed)) - 8]


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fastq_text():
    seq, meta = M.synth(3, genome_len=6000, depth=20, len_lo=100, len_hi=150)[:2]
    rng = np.random.default_rng(4)
    recs = []
    for i in range(seq.shape[0]):
        L = int(meta[i])
        q = np.where(rng.random(L) < 0.7, ord('F'), rng.integers(35, 75, L)).astype(np.uint8)
        recs.append(b'@SRR0001.%d %d/1\n%s\n+\n%s\n' % (i + 1, i + 1, seq[i, :L].tobytes(), q.tobytes()))
    text = b''.join(recs)
    assert len(text) > 2 * BLOCK + 1
    return text


@pytest.mark.parametrize('n', [1, 2, 65279, 65280, 65281, 2 * 65280 + 1])
def test_sizes_around_the_block(fastq_text, n):
    got = check(fastq_text[:n])
    assert len(got) == (n + BLOCK - 1) // BLOCK


@pytest.mark.parametrize('n', [1, 4095, 4096, 4097, 3 * 4096 + 1])
def test_blocks_of_4096(fastq_text, n):
    got = check(fastq_text[1000:1000 + n], 4096)
    assert len(got) == (n + 4095) // 4096
    assert check(fastq_text[:9], 1) == [(0, 32)] * 9                  # the smallest block: a stored byte each


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_equal_bytes_are_chained_matches():
    (btype, size), = check(b'a' * BLOCK)
    assert btype == 2 and size < 2048


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_two_symbols_and_no_distance_code():
    """Five equal bytes: no dynamic header is smaller than five stored bytes (the header alone is longer), so the block is
    stored, as the fallback rule says.  A hundred equal bytes inside the first tile meet no earlier tile to match: one literal
    symbol and the end of block, one bit each, and a distance alphabet of ONE code of zero bits -- unused."""
    assert check(b'a' * 5) == [(0, 5 + 31)]
    text = b'a' * 100
    (btype, size), = check(text)
    assert btype == 2 and size < 18 + 8 + 32
    ll, dist, cl = dynamic_header(payload_of(deflate(text)[0]))
    assert [s for s, l in enumerate(ll) if l] == [ord('a'), 256] and ll[ord('a')] == ll[256] == 1
    assert dist == [0]
    assert max(cl) <= 7


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_a_repeated_line_is_matched_to_the_last_byte():
    line = np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8).tobytes()
    text = line * 1000
    assert len(text) == 64000
    for block_bytes in (BLOCK, 4096 + 37):                           # 4133: every block ends inside a line
        got = check(text, block_bytes)
        assert all(btype == 2 for btype, _ in got[:-1])
        if block_bytes == BLOCK:
            assert sum(size for _, size in got) < len(text) // 8      # a literal-only code cannot go below one bit a byte
    got = check((line * 1021)[:BLOCK])                               # a full block whose end falls inside a line
    assert got[0][1] < BLOCK // 8


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_distances_stop_at_32768():
    rng = np.random.default_rng(2)
    text = bytearray(rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes())
    seg, far = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(), rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    text[100:1100] = seg
    text[100 + 32768:1100 + 32768] = seg                             # distance exactly 32768: the longest a match may reach
    text[20000:20300] = far
    text[20000 + 32769:20300 + 32769] = far                          # 32769: must stay literals -- inflating (check) refuses
    text[2000:2300] = far[::-1]                                      # a distance too far back
    text[2000 + 40000:2300 + 40000] = far[::-1]                      # and further
    (btype, size), = check(bytes(text))
    # random bytes alone are stored (test 7): only the 1000 bytes matched at 32768 make the coded form the smaller one
    assert btype == 2 and size < BLOCK + 31 - 500


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_code_lengths_are_limited_to_15_bits():
    # 245 byte values seen once (with the end of block a subtree of weight 246, eight levels deep) under a Fibonacci run that
    # starts above half that weight: every member is merged alone, one level each
    fib = [130, 250]
    while len(fib) < 11:
        fib.append(fib[-1] + fib[-2])
    freq = fib + [1] * (256 - len(fib))
    assert len(freq) == 256 and sum(freq) == 47565 <= BLOCK
    import heapq
    heap = [(f, 0) for f in freq + [1]]                              # ... with the end of block: (weight, depth of the subtree)
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    assert heap[0][1] > 15                                           # unlimited Huffman lengths exceed 15 bits here
    text = np.repeat(np.arange(256, dtype=np.uint8), freq)
    np.random.default_rng(6).shuffle(text)
    (btype, size), = check(text.tobytes())
    assert btype == 2
    ll, dist, cl = dynamic_header(payload_of(deflate(text.tobytes())[0]))
    used = [l for l in ll if l]
    assert len(used) >= 257 and max(used) <= 15                      # every byte value and the end of block, none over the limit
    assert sum(2.0 ** -l for l in used) == 1.0                       # and the code is complete
    assert max(cl) <= 7


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_random_bytes_are_stored():
    text = np.random.default_rng(8).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()
    assert check(text) == [(0, BLOCK + 31)]
    packed = deflate(text)[0]
    assert packed[18:23] == b'\x01' + struct.pack('<HH', BLOCK, BLOCK ^ 0xFFFF) and packed[23:-8] == text


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_fastq_text_is_coded_and_shorter(fastq_text):
    text = fastq_text[:3 * BLOCK]
    got = check(text)
    assert len(got) == 3 and all(btype == 2 and size < BLOCK // 2 for btype, size in got)
    small = check(text[:5 * 4096], 4096)
    assert all(btype == 2 and size < 4096 for btype, size in small)


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_the_bytes_do_not_depend_on_the_call(fastq_text, monkeypatch):
    text = fastq_text[:2 * BLOCK + 1]
    first = deflate(text)[0]
    assert deflate(text)[0] == first
    assert deflate(text, host=True) == first
    monkeypatch.setenv('KBBQ_STAGE_MB', '1')                         # slabs of five blocks
    long = (fastq_text * 6)[:12 * BLOCK + 77]
    assert deflate(long, host=True) == deflate(long)[0]
    assert deflate(long[:20000], 1000, host=True) == deflate(long[:20000], 1000)[0]
    # a block's bytes depend on its own text alone: not on its place, nor on how many workgroups share the work
    sizes = deflate(text)[1]
    assert deflate(text[BLOCK:2 * BLOCK])[0] == first[sizes[0]:sizes[0] + sizes[1]]


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_refusals(fastq_text):
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    lib, ctx = N.load(), dev.context()
    text = np.frombuffer(fastq_text[:1000], dtype=np.uint8)
    d_text = torch.from_numpy(text.copy()).cuda()
    d_blocks = torch.zeros(N.BGZF_SLOT + 16, dtype=torch.uint8, device='cuda')
    d_sizes = torch.zeros(4, dtype=torch.int32, device='cuda')
    d_packed = torch.zeros(2000, dtype=torch.uint8, device='cuda')
    total = ctypes.c_size_t(5)

    def dev_call(n=1000, block_bytes=BLOCK, t=d_text, b=d_blocks, s=d_sizes, p=d_packed, h=ctx.handle, r=ctypes.byref(total)):
        return lib.kbbq_bgzf_deflate_dev(h, N.ptr(t), n, block_bytes, N.ptr(b), N.ptr(s), N.ptr(p), r)
    for bad in (0, -5, 65281):
        assert dev_call(block_bytes=bad) == N.KBBQ_E_ARG and 'block_bytes' in N.last_error()
    assert dev_call(n=-1) == N.KBBQ_E_ARG
    for kw in (dict(t=None), dict(b=None), dict(s=None), dict(p=None), dict(h=None), dict(r=None)):
        assert dev_call(**kw) == N.KBBQ_E_ARG, kw
    assert dev_call(b=d_blocks[1:]) == N.KBBQ_E_ARG and 'aligned' in N.last_error()
    assert dev_call(n=0, t=None, b=None, s=None, p=None) == N.KBBQ_OK and total.value == 0     # nothing to write
    out = np.zeros(2000, dtype=np.uint8)
    cap = int(lib.kbbq_bgzf_bound(1000, BLOCK))
    assert cap == 1031
    assert lib.kbbq_bgzf_deflate(ctx.handle, N.ptr(text), 1000, BLOCK, N.ptr(out), cap - 1, ctypes.byref(total)) == N.KBBQ_E_ARG
    assert 'kbbq_bgzf_bound' in N.last_error() and not out.any()
    assert lib.kbbq_bgzf_deflate(ctx.handle, N.ptr(text), 1000, 0, N.ptr(out), cap, ctypes.byref(total)) == N.KBBQ_E_ARG
    assert lib.kbbq_bgzf_deflate(ctx.handle, None, 1000, BLOCK, N.ptr(out), cap, ctypes.byref(total)) == N.KBBQ_E_ARG
    assert lib.kbbq_bgzf_deflate(ctx.handle, N.ptr(text), 0, BLOCK, None, 0, ctypes.byref(total)) == N.KBBQ_OK and total.value == 0
    with pytest.raises(ValueError, match='block_bytes'):
        N.check(dev_call(block_bytes=0))
    assert dev_call() == N.KBBQ_OK and gzip.decompress(d_packed.cpu().numpy()[:total.value].tobytes()) == text.tobytes()
