"""The inputs of tests/test_gpu_bgzf_edges.py, designed on the CPU against the host model (tests/bgzf_model.py) so that each
enters one path of csrc/kbbq_bgzf.h that ordinary text does not.  test_bgzf_model_host.py checks on the model that each does
what it is for; the GPU test then asks the same of the kernel's own bytes.

The four full-size blocks are the result of a search (words re-drawn until every planted match lands) and are kept as files:
`python tests/bgzf_cases.py` writes them again to tests/golden/bgzf_*.bin.  Everything else is built on the fly."""
import functools
import os

import numpy as np

import bgzf_model as B

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BLOCK = B.BLOCK_MAX


# ---- several blocks per workgroup ----------------------------------------------------------------------------------------
WG_BLOCK = 1101                                            # three tiles; 1101 is odd, so block starts fall on every alignment
WG_KINDS = ('rich', 'poor', 'random', 'dna')


def wg_kind(b, cus):
    """Kind of block b: blocks b and b + cus, which one workgroup codes one after the other, are of different kinds."""
    return WG_KINDS[(b + b // cus) % 4]


def wg_piece(b, cus, n=WG_BLOCK):
    rng = np.random.default_rng(1000 + b)
    kind = wg_kind(b, cus)
    if kind == 'rich':                                     # all 256 byte values in the first tile, then pieces of it again
        tile = np.concatenate([rng.permutation(256), rng.permutation(256)]).astype(np.uint8)
        out = [tile]
        while sum(map(len, out)) < n:
            a, l = int(rng.integers(0, 480)), int(rng.integers(8, 60))
            out.append(tile[a:a + l])
        return np.concatenate(out)[:n].tobytes()
    if kind == 'poor':                                     # one byte value: literals in the first tile, then three matches
        return bytes([65 + b % 26]) * n
    if kind == 'random':
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), n).tobytes()


def wg_text(nblocks, cus):
    """nblocks blocks of WG_BLOCK bytes, the last one 37 bytes short of full"""
    return b''.join(wg_piece(b, cus) for b in range(nblocks - 1)) + wg_piece(nblocks - 1, cus, WG_BLOCK - 37)


# ---- more blocks than bz_scan_sizes has threads --------------------------------------------------------------------------
MANY_BLOCK = 101


def many_text(nblocks):
    """Blocks of 101 bytes, random (stored, 132 bytes) or of four letters (coded, about 50), in no regular order; the last one
    of 11 bytes."""
    rng = np.random.default_rng(nblocks)
    out = []
    for b in range(nblocks):
        n = MANY_BLOCK if b < nblocks - 1 else 11
        if rng.random() < 0.45:
            out.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        else:
            out.append(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), n).tobytes())
    return b''.join(out)


# ---- a literal-only block whose code-length code needs limiting ----------------------------------------------------------
# (byte value, count): found by cl_limit_search(0).  498 bytes in one tile, so no matches and exact counts; 128 byte values.
CL_LIMIT_FREQ = (
    (2, 1), (6, 6), (7, 1), (8, 3), (9, 8), (12, 3), (13, 3), (17, 5), (18, 1), (19, 3), (20, 11), (21, 27), (28, 4), (29,
    3), (30, 3), (32, 1), (34, 2), (36, 3), (37, 1), (38, 5), (40, 2), (41, 13), (42, 2), (44, 1), (45, 2), (46, 1), (47,
    6), (48, 1), (50, 8), (52, 6), (57, 3), (62, 3), (63, 5), (64, 4), (65, 3), (66, 1), (71, 1), (72, 1), (73, 7), (75, 3),
    (77, 5), (79, 2), (80, 1), (84, 3), (85, 2), (86, 4), (87, 1), (88, 4), (92, 4), (94, 1), (95, 3), (98, 2), (99, 1),
    (100, 2), (102, 5), (103, 2), (104, 15), (108, 1), (109, 2), (110, 1), (112, 5), (115, 25), (116, 1), (117, 3), (118,
    5), (122, 2), (123, 6), (124, 4), (129, 2), (130, 1), (131, 1), (135, 8), (137, 2), (139, 4), (140, 2), (142, 5), (145,
    1), (148, 1), (160, 5), (163, 1), (164, 2), (167, 3), (169, 4), (175, 2), (176, 1), (177, 2), (179, 6), (183, 5), (184,
    3), (185, 10), (186, 5), (187, 1), (191, 2), (192, 4), (193, 1), (197, 1), (200, 1), (201, 3), (203, 3), (204, 1), (205,
    4), (206, 7), (208, 4), (209, 8), (214, 1), (215, 3), (217, 5), (218, 5), (220, 2), (223, 3), (225, 4), (226, 14), (227,
    7), (228, 1), (230, 3), (231, 1), (232, 1), (233, 1), (234, 18), (235, 1), (236, 14), (239, 3), (241, 1), (246, 2),
    (249, 1), (252, 4), (253, 2), (254, 6))


def _cl_depth(freq):
    ll, code = [0] * 286, [0] * 286
    B.build_code(list(freq) + [1] + [0] * 29, 15, ll, code)
    fc = [0] * 19
    for s, _ in B._cl_stream(ll[:257] + [0]):
        fc[s] += 1
    return B.build_code(fc, 7, [0] * 19, [0] * 19), fc


def cl_limit_search(seed, most=500):
    """Hill-climb over the counts of the byte values of a block of at most `most` bytes for a code-length code deeper than 7
    bits before limiting, in a block that is still sent coded."""
    rng = np.random.default_rng(seed)
    freq = np.zeros(256, dtype=np.int64)
    freq[rng.choice(256, 80, replace=False)] = np.maximum(1, (rng.pareto(1.0, 80) * 2).astype(np.int64))
    while freq.sum() > most:
        freq[freq.argmax()] //= 2

    def score(f):
        deep, fc = _cl_depth(f)
        srt, acc, fib = sorted(x for x in fc if x), 0, 0
        for i, x in enumerate(srt):                        # how far the counts of the code-length symbols run Fibonacci-like
            fib += 1 if i >= 2 and acc <= x else 0
            acc += x
        if deep <= 7:
            return 0, fib, 0
        rec = B.deflate_block(cl_limit_text(f))[1]         # deep enough: now towards a block smaller coded than stored
        return 1, 0, int(f.sum()) + 5 - ((rec['header_bits'] + rec['body_bits'] + 7) >> 3)
    cur = score(freq)
    for _ in range(40000):
        g = freq.copy()
        for _ in range(int(rng.integers(1, 4))):
            i = int(rng.integers(256))
            g[i] = max(0, g[i] + int(rng.choice([-8, -3, -2, -1, 1, 2, 3, 8])))
        if not 1 <= g.sum() <= most:
            continue
        sc = score(g)
        if sc >= cur:
            freq, cur = g, sc
        if cur[0] and cur[2] > 0:
            return [(int(i), int(f)) for i, f in enumerate(freq) if f]
    return None


def cl_limit_text(freq=None):
    if freq is None:
        freq = np.zeros(256, dtype=np.int64)
        for i, f in CL_LIMIT_FREQ:
            freq[i] = f
    text = np.repeat(np.arange(256, dtype=np.uint8), np.asarray(freq))
    np.random.default_rng(7).shuffle(text)
    return text.tobytes()


# ---- planted matches -----------------------------------------------------------------------------------------------------
class Planter:
    """A block of random bytes with planted matches: a word of L bytes at `a` and again at a + D, the bytes around the copy
    made to differ from those around the word, so that the greedy parse lands on the copy and the match is exactly (L, D) -- if
    the word's hash head still names `a` when the copy's tile is matched.  16,384 heads serve 65,280 positions, so a far word
    is often displaced; settle() draws such words again until every plant lands."""

    def __init__(self, n, seed):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.s = self.rng.integers(0, 256, n, dtype=np.uint8)
        self.used = np.zeros(n + 2, dtype=bool)
        self.plants = []

    def free(self, a, L, D):
        if a < 1 or a + D + L + 1 > self.n or D < 1:
            return False
        if D < L + 2 or (a + D) // B.TILE <= a // B.TILE:   # apart, and the word in an earlier tile than its copy
            return False
        return not self.used[a - 1:a + L + 1].any() and not self.used[a + D - 1:a + D + L + 1].any()

    def put(self, a, L, D):
        assert self.free(a, L, D), (a, L, D)
        self.used[a - 1:a + L + 1] = True
        self.used[a + D - 1:a + D + L + 1] = True
        self.plants.append((a, L, D))
        self.draw(len(self.plants) - 1)

    def draw(self, i):
        a, L, D = self.plants[i]
        w = self.rng.integers(0, 256, L, dtype=np.uint8)
        self.s[a:a + L] = w
        self.s[a + D:a + D + L] = w
        self.s[a + D - 1] = self.s[a - 1] ^ 0x55
        if a + D + L < self.n:
            self.s[a + D + L] = self.s[a + L] ^ 0xAA

    def fit(self, L, D, start=1):
        """put() at the first free place from `start` on; returns the place after it, or None"""
        for a in range(start, self.n - D - L):
            if self.free(a, L, D):
                self.put(a, L, D)
                return a + L + 1
        return None

    def settle(self, rounds=200):
        for _ in range(rounds):
            pos, lens, dists, _ = B.lz_parse(self.s.tobytes())
            got = {p: (l, d) for p, l, d in zip(pos, lens, dists)}
            bad = [i for i, (a, L, D) in enumerate(self.plants) if got.get(a + D) != (L, D)]
            if not bad:
                return self.s.tobytes()
            for i in bad:
                self.draw(i)
        raise AssertionError('%d plants do not land' % len(bad))


THREE_NEAR = ((18, 24), (19, 48), (20, 96), (21, 192), (22, 384), (23, 768), (24, 1536))   # (distance symbol, copies)


def design_three_words():
    """Tokens of 34 bits and more: 24 words of 131..257 bytes (length symbols 281..284, 5 extra bits, three to nine uses each
    among some forty thousand tokens: codes of 12 to 14 bits) copied 16,385..32,768 bytes on (13 extra bits), three of them in
    distance symbol 28 and 21 in 29; and 3,048 words of four bytes copied 513..6,144 bytes on, twice as many in each distance
    symbol as in the one before, which puts the two far symbols nine levels down."""
    pl = Planter(BLOCK, 31)
    rng = np.random.default_rng(32)
    at = 1
    for i in range(24):
        L = 131 + 10 * i if i < 3 else 163 + 10 * (i - 3) if i < 6 else 195 + ((i - 6) * 62) // 17
        D = int(rng.integers(16385, 24577)) if i in (0, 3, 10) else int(rng.integers(24577, 32769 - 600))
        at = pl.fit(L, D, at)
        assert at is not None
    for sym, count in reversed(THREE_NEAR):
        D, at = int(rng.integers(B.DIST_LOW[sym], B.DIST_HIGH[sym] + 1)), 1
        for _ in range(count):
            at = pl.fit(4, D, at)
            assert at is not None, (sym, count)
    return pl.settle()


DIST_LIMIT_COUNTS = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597)
# the symbols in ascending order of their counts: the rarest below distance 513, where a copy must sit at the start of a tile;
# then the far ones, whose words are the most often displaced; the frequent ones next to their copies
DIST_LIMIT_SYMS = (13, 14, 15, 16, 17, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18)


def design_dist_limit():
    """A distance code deeper than 15 bits before limiting: words of four bytes, each copied once, the copies' distances in 17
    symbols whose counts are the Fibonacci numbers 1, 1, 2, ... 1597 -- the least counts with a Huffman tree 16 deep."""
    pl = Planter(BLOCK, 41)
    rng = np.random.default_rng(42)
    for count, sym in zip(DIST_LIMIT_COUNTS, DIST_LIMIT_SYMS):
        lo, hi = B.DIST_LOW[sym], B.DIST_HIGH[sym]
        if sym < 18:                                       # the copy at a tile's first bytes, the word less than a tile before
            for _ in range(count):
                tile = 2 + len(pl.plants) * 9
                D = int(rng.integers(lo, hi + 1))
                pl.put(tile * B.TILE + 1 - D, 4, D)
            continue
        D, at = int(rng.integers(lo, min(hi, lo + 200) + 1)), 1
        for _ in range(count):
            at = pl.fit(4, D, at)
            assert at is not None, (sym, count)
    return pl.settle()


LL_LIMIT_COUNTS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144)   # of the length symbols 258 .. 268 (4 .. 17 bytes); the end of block is the other 1


def design_ll_limit():
    """A literal/length code deeper than 15 bits before limiting, with exact counts: the end of block and eleven length symbols whose counts run
    1, 1, 2, ... 144 (eleven levels) below the 256 byte values of random text, about 250 each (eight levels more).  A shuffled
    text with such counts of byte values does not do it: its frequent bytes repeat, the parse finds thousands of matches, and the
    counts are no longer the ones designed (the model shows 13 levels for the text of test_gpu_bgzf.py's sixth case)."""
    pl = Planter(BLOCK, 61)
    rng = np.random.default_rng(62)
    at = 1
    for i, count in enumerate(LL_LIMIT_COUNTS):
        L = B.LEN_BASE[1 + i]
        for _ in range(count):
            at = pl.fit(L, int(rng.integers(513, 1500)), at)
            assert at is not None
    return pl.settle()


def design_far_bounds():
    """The lowest and the highest distance of the symbols 18..29 (513 .. 32768), each with a word of another length; and a word
    of 258 bytes whose copy starts at position 511 of a tile, so that 257 bytes are carried into the next."""
    pl = Planter(BLOCK, 51)
    pl.put(1, 258, 2 * B.TILE - 1 - 1)                     # the copy at 1023
    at, L = 300, 5
    for sym in range(29, 17, -1):
        for D in (B.DIST_HIGH[sym], B.DIST_LOW[sym]):
            at = pl.fit(L, D, at)
            assert at is not None
            L += 9
    return pl.settle()


NEAR_BLOCK = 771                                           # a tile, a match of up to 258 bytes, a breaker
NEAR_DISTS = sorted(set(d for d in B.DIST_LOW + B.DIST_HIGH if d <= 512))


def near_pair(b):
    """(length, distance) planted in block b of near_text(): every length 4..258, and in turn every distance up to 512 that is
    the lowest or the highest of its symbol."""
    return 4 + b, NEAR_DISTS[b % len(NEAR_DISTS)]


def near_text():
    """255 blocks of 771 bytes: text of period D as far as position 512 + L, then one other byte value.  The first tile is literals, the
    match at 512 finds the same phase D bytes back and stops after L bytes."""
    out = []
    for b in range(255):
        L, D = near_pair(b)
        rng = np.random.default_rng(7000 + b)
        while True:
            w = rng.permutation(256)[:D] if D <= 256 else np.concatenate([rng.permutation(256), rng.permutation(256)])[:D]
            piece = np.resize(w.astype(np.uint8), B.TILE + L)
            rest = np.full(NEAR_BLOCK - len(piece), w[(B.TILE + L) % D] ^ 0x55, dtype=np.uint8)   # cheap literals: the block stays coded
            piece = np.concatenate([piece, rest]).tobytes()
            pos, lens, dists, _ = B.lz_parse(piece)
            if (B.TILE, L, D) in set(zip(pos, lens, dists)):
                break
        out.append(piece)
    return b''.join(out)


# ---- CRC strips and the two copy-in paths --------------------------------------------------------------------------------
def crc_sizes():
    """1..64; either side of every change of the strip length; k strips exactly and a byte either side, for strips of 4 and of
    12 bytes."""
    ns = set(range(1, 65))
    changes = [n for n in range(1, BLOCK) if B.strip_length(n) != B.strip_length(n + 1)]
    assert changes[:3] == [2048, 6144, 10240] and len(changes) == 16
    for n in changes:
        ns |= {n, n + 1}
    for L, ks in ((4, (100, 511, 512)), (12, (171, 300, 511, 512))):
        for k in ks:
            for n in (k * L - 1, k * L, k * L + 1):
                if B.strip_length(n) == L:
                    ns.add(n)
    ns.add(BLOCK)
    return sorted(ns)


@functools.lru_cache(maxsize=None)
def crc_base():
    return np.random.default_rng(77).integers(0, 256, BLOCK + 16, dtype=np.uint8)


# ---- what each case is for, read from decoded blocks (bgzf_model.verify) -------------------------------------------------
def kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


def _matches(blk):
    return [t for _, _, t in blk['tokens'] if isinstance(t, tuple)]


def props_wg(blocks, cus):
    """rich: every literal and the end of block have a code, and there are matches; poor: a literal, the end of block and at
    most three lengths; random: stored; and no block has the kind of the one its workgroup coded before it."""
    seen = set()
    for b, blk in enumerate(blocks):
        kind = wg_kind(b, cus)
        seen.add(kind)
        assert b < cus or kind != wg_kind(b - cus, cus)
        if kind == 'random':
            assert blk['btype'] == 0, b
            continue
        assert blk['btype'] == 2, b
        used = [s for s, l in enumerate(blk['ll']) if l]
        if kind == 'rich':
            assert all(blk['ll'][:257]) and len(_matches(blk)) >= 5, b
        elif kind == 'poor' and b < len(blocks) - 1:
            assert used[:2] == [65 + b % 26, 256] and 3 <= len(used) <= 5 and len(_matches(blk)) == 3, (b, used)
            assert 1 <= sum(1 for l in blk['d'] if l) <= 3, b
    assert seen == set(WG_KINDS)


def props_many(blocks, sizes):
    kinds = [blk['btype'] for blk in blocks]
    assert set(kinds) == {0, 2}
    assert len(set(int(x) for x in sizes[:-1])) > 2         # the offsets are no arithmetic progression
    runs = sum(1 for a, b in zip(kinds, kinds[1:]) if a != b)
    assert runs > len(blocks) // 4                          # stored and coded alternate, irregularly


def props_three_words(blocks):
    rec = B.paths(blocks[0])
    assert blocks[0]['btype'] == 2
    assert rec['three_words'] >= 1 and rec['max_token_bits'] >= 40, (rec['three_words'], rec['max_token_bits'])
    assert sum(1 for _, bits, _ in blocks[0]['tokens'] if bits >= 34) >= 20
    return rec


def props_cl_limit(blocks):
    blk = blocks[0]
    assert blk['btype'] == 2 and not _matches(blk) and len(blk['tokens']) <= B.TILE
    deep = B.unlimited_depth(B.cl_freq(blk))
    assert deep > 7 and max(blk['cl']) <= 7 and kraft(blk['cl']) == 1.0, (deep, blk['cl'])
    return deep


def props_ll_limit(blocks):
    blk = blocks[0]
    rec = B.paths(blk)
    deep = B.unlimited_depth(rec['freq_ll'])
    used = [l for l in blk['ll'] if l]
    assert blk['btype'] == 2 and deep > 15 and max(used) <= 15 and kraft(used) == 1.0, (deep, max(used))
    assert [bool(l) for l in blk['ll']] == [bool(f) for f in rec['freq_ll'][:len(blk['ll'])]]
    return deep


def props_dist_limit(blocks):
    blk = blocks[0]
    rec = B.paths(blk)
    deep = B.unlimited_depth(rec['freq_d'])
    assert blk['btype'] == 2 and sum(1 for f in rec['freq_d'] if f) >= 17
    assert deep > 15 and max(blk['d']) <= 15 and kraft(blk['d']) == 1.0, (deep, blk['d'])
    assert [bool(l) for l in blk['d']] == [bool(f) for f in rec['freq_d'][:len(blk['d'])]]
    return deep


def props_bounds(near_blocks, far_blocks):
    lengths, dists = set(), set()
    for b, blk in enumerate(near_blocks):
        rec = B.paths(blk)
        assert near_pair(b) in rec['pairs'], (b, near_pair(b))
        lengths |= rec['lengths']
        dists |= rec['dists']
    rec = B.paths(far_blocks[0])
    lengths |= rec['lengths']
    dists |= rec['dists']
    assert lengths >= set(range(4, 259)), sorted(set(range(4, 259)) - lengths)
    want = set(B.DIST_LOW + B.DIST_HIGH)
    assert len(want) == 56 and {1, 32768} <= want
    assert dists >= want, sorted(want - dists)
    assert 258 in rec['starts_511'] and rec['max_carry'] == 257


# ---- the texts of tests/test_gpu_bgzf.py ---------------------------------------------------------------------------------
def existing_texts():
    """(name, text, block_bytes) of the cases tests/test_gpu_bgzf.py runs, FASTQ-like text in place of its synthetic reads."""
    rng = np.random.default_rng(4)
    recs = []
    for i in range(1300):
        L = int(rng.integers(100, 151))
        seq = rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), L).tobytes()
        q = np.where(rng.random(L) < 0.7, ord('F'), rng.integers(35, 75, L)).astype(np.uint8).tobytes()
        recs.append(b'@SRR0001.%d %d/1\n%s\n+\n%s\n' % (i + 1, i + 1, seq, q))
    fastq = b''.join(recs)
    assert len(fastq) > 2 * BLOCK + 1
    out = [('fastq %d' % n, fastq[:n], BLOCK) for n in (1, 2, 65279, 65280, 65281, 2 * 65280 + 1)]
    out += [('fastq 4096 %d' % n, fastq[1000:1000 + n], 4096) for n in (1, 4095, 4096, 4097, 3 * 4096 + 1)]
    out += [('bytes alone', fastq[:9], 1), ('equal bytes', b'a' * BLOCK, BLOCK), ('five', b'a' * 5, BLOCK), ('hundred', b'a' * 100, BLOCK)]
    line = np.random.default_rng(1).integers(0, 256, 64, dtype=np.uint8).tobytes()
    out += [('lines', line * 1000, BLOCK), ('lines 4133', line * 1000, 4133), ('lines cut', (line * 1021)[:BLOCK], BLOCK)]
    rng = np.random.default_rng(2)
    text = bytearray(rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes())
    seg, far = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(), rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    text[100:1100] = seg
    text[100 + 32768:1100 + 32768] = seg
    text[20000:20300] = far
    text[20000 + 32769:20300 + 32769] = far
    out.append(('32768', bytes(text), BLOCK))
    fib = [130, 250]
    while len(fib) < 11:
        fib.append(fib[-1] + fib[-2])
    text = np.repeat(np.arange(256, dtype=np.uint8), fib + [1] * 245)
    np.random.default_rng(6).shuffle(text)
    out.append(('15 bits', text.tobytes(), BLOCK))
    out.append(('random', np.random.default_rng(8).integers(0, 256, BLOCK, dtype=np.uint8).tobytes(), BLOCK))
    return out


GOLDEN = dict(three_words=design_three_words, ll_limit=design_ll_limit, dist_limit=design_dist_limit, far_bounds=design_far_bounds)


@functools.lru_cache(maxsize=None)
def golden(name):
    with open(os.path.join(GOLD, 'bgzf_%s.bin' % name), 'rb') as fh:
        return fh.read()


if __name__ == '__main__':
    for name, design in GOLDEN.items():
        text = design()
        with open(os.path.join(GOLD, 'bgzf_%s.bin' % name), 'wb') as fh:
            fh.write(text)
        rec = B.deflate_block(text)[1]
        print(name, len(text), rec['btype'], rec['limited'], rec['depth'], rec['max_token_bits'], rec['three_words'],
              rec['long_tokens'], rec['max_carry'])
