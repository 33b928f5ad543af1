"""
Probe models, reads and a plain reference for K2 (the apply kernels): no GPU, no product code, no oracle.

A solved model is nearly flat -- its cycle and context deltas are -1, 0 or 1 almost everywhere -- so a kernel that reads a
neighbouring LUT column, forgets the second mate's mirror or swaps the two bases of a context still returns the right byte
for almost every base.  The models here are built the other way round: the OUTPUT BYTE names the index that was looked
up, and the entries sit on the ends of what the LUT's contract allows (int8 entries, cycle + context + 33 in 0 .. 255).

    reference_apply   the reference's rule (compare_reads.py:320-328) as an int64 gather
    fast_range        the blob's two range flags, stated in NumPy
    probes            the probe models for any (R, S2), all inside the fast range
    one_past_*        the context probe with one cell that leaves the range, and the int8 misfit
    reads             host planes that reach every quality, context and column on counted bases
    MISTAKES          index mistakes a kernel could make, for the discriminating-power test of the probes themselves

A model is the tuple (meanq [R], rgdq [R], qdq [R, Qt], posdq [R, Qt, S2], dinucdq [R, Qt, 17]) of int64 arrays, as
`oracle.apply` and `_device.build_lut` take it.  LUT terms: the CYCLE entry of (r, q, col) is meanq[r] + rgdq[r] +
qdq[r, q] + posdq[r, q, col], the CONTEXT entry of (r, q, ctx) is dinucdq[r, q, ctx]; every builder below starts from
the entries it wants and spreads the cycle entry over all four arrays, so none of them is zero.
"""
import numpy as np

QT = 43                      # quality rows of the model: bytes 33 .. 75
D = 17                       # 16 dinucleotides and the "no context" column
MINSCORE = 6

_CODE = np.full(256, -1, dtype=np.int64)
for _k, _c in enumerate('ATGC'):
    _CODE[ord(_c)] = _k
_LETTER = np.zeros(256, dtype=bool)
_LETTER[[ord(c) for c in 'ACGTN']] = True


# ---------------------------------------------------------------------------------------------------- reference
class Lookups:
    """The indices the rule looks up for every counted base of a batch: flat arrays over the counted bases."""
    pass


def lookups(seq, qual, meta, S2, minscore=MINSCORE):
    """Which (read group r, quality q, column col, context ctx) every counted base looks up; `row`, `pos` say where the
    base is, `second` whether its read is a second mate.  `inside` [n, pitch]: the bytes within the reads."""
    seq, qual = np.asarray(seq), np.asarray(qual)
    meta = np.asarray(meta).astype(np.int64)
    n, pitch = seq.shape
    lens, rg, second = meta & 0xFFFF, (meta >> 16) & 0x7FFF, (meta >> 31) & 1
    i = np.arange(pitch, dtype=np.int64)[None, :]
    inside = i < lens[:, None]
    if not _LETTER[seq[inside]].all():
        raise TypeError('a base outside ACGTN')
    q = qual.astype(np.int64) - 33
    counted = inside & (q >= minscore)
    cur = _CODE[seq]
    prev = np.full_like(cur, -1)
    prev[:, 1:] = cur[:, :-1]                                        # position 0 has no previous base
    ctx = np.where((cur >= 0) & (prev >= 0), 4 * prev + cur, D - 1)
    col = np.where(second[:, None] == 1, S2 - 1 - i, i)
    L = Lookups()
    L.inside, L.counted = inside, counted
    L.row, L.pos = np.nonzero(counted)
    L.r, L.second = rg[L.row], second[L.row]
    L.q, L.col, L.ctx = q[counted], col[counted], ctx[counted]
    L.S2 = S2
    return L


def values(model, r, q, col, ctx):
    """meanq[r] + rgdq[r] + qdq[r, q] + posdq[r, q, col] + dinucdq[r, q, ctx]: IndexError where the reference's is."""
    meanq, rgdq, qdq, posdq, dinucdq = (np.asarray(x, dtype=np.int64) for x in model)
    R, Qt, S2 = posdq.shape
    if len(r) and (r.max() >= R or q.max() >= Qt or col.min() < 0 or col.max() >= S2):
        raise IndexError('a read group, quality or column beyond the model')
    return meanq[r] + rgdq[r] + qdq[r, q] + posdq[r, q, col] + dinucdq[r, q, ctx]


def reference_apply(seq, qual, meta, meanq, rgdq, qdq, posdq, dinucdq, minscore=MINSCORE):
    """The new quality BYTES (value + 33, int64 [n, pitch], not clamped: a one-past model gives -1 or 256): a base of raw
    quality q < minscore keeps its byte; otherwise column = position (first mate) or S2 - 1 - position (second),
    context = 4 code(prev) + code(cur) with A0 T1 G2 C3, column D - 1 at position 0 or next to an N; bytes at and
    beyond the read length are 0."""
    model = (meanq, rgdq, qdq, posdq, dinucdq)
    L = lookups(seq, qual, meta, np.asarray(posdq).shape[2], minscore)
    out = np.where(L.inside, np.asarray(qual).astype(np.int64), 0)
    out[L.row, L.pos] = values(model, L.r, L.q, L.col, L.ctx) + 33
    return out


# ---------------------------------------------------------------------------------------------------- range predicate
def entries(model):
    """(cycle [R, Qt, S2], context [R, Qt, 17]) LUT entries of a model."""
    meanq, rgdq, qdq, posdq, dinucdq = (np.asarray(x, dtype=np.int64) for x in model)
    return (meanq + rgdq)[:, None, None] + qdq[:, :, None] + posdq, dinucdq


def fast_range(model, minscore=MINSCORE):
    """The blob's flags: 1 when an entry does not fit int8, 2 when, for a model row (r, q >= minscore), min cycle +
    min context + 33 < 0 or max cycle + max context + 33 > 255.  0: the fast kernels may run without clamping."""
    cyc, ctx = entries(model)
    flags = 0
    if min(cyc.min(), ctx.min()) < -128 or max(cyc.max(), ctx.max()) > 127:
        flags |= 1
    lo = cyc.min(axis=2) + ctx.min(axis=2) + 33
    hi = cyc.max(axis=2) + ctx.max(axis=2) + 33
    if (lo[:, minscore:] < 0).any() or (hi[:, minscore:] > 255).any():
        flags |= 2
    return flags


# ---------------------------------------------------------------------------------------------------- models
def model_of(cyc, ctx):
    """The five model arrays whose LUT entries are `cyc` [R, Qt, S2] and `ctx` [R, Qt, 17]."""
    cyc, ctx = np.asarray(cyc, dtype=np.int64), np.asarray(ctx, dtype=np.int64)
    R, Qt, _ = cyc.shape
    r, q = np.arange(R, dtype=np.int64), np.arange(Qt, dtype=np.int64)
    meanq = 15 + 3 * r
    rgdq = 2 - r
    qdq = (3 * q[None, :] + r[:, None]) % 7 - 3
    posdq = cyc - (meanq + rgdq)[:, None, None] - qdq[:, :, None]
    return meanq, rgdq, qdq, posdq, ctx.copy()


def _grid(R, S2):
    return (np.arange(R, dtype=np.int64)[:, None, None], np.arange(QT, dtype=np.int64)[None, :, None],
            np.arange(S2, dtype=np.int64)[None, None, :])


def column_probe(R, S2, m):
    """Output byte (col + 5 q + 17 r) mod m: contexts 0."""
    r, q, col = _grid(R, S2)
    return model_of((col + 5 * q + 17 * r) % m - 33, np.zeros((R, QT, D), dtype=np.int64))


def context_probe(R, S2):
    """Cycle entry 95 everywhere; the 16 dinucleotides -128, -112 .. 112, no context 127: output bytes 0, 16 .. 240, 255."""
    ctx = np.empty((R, QT, D), dtype=np.int64)
    ctx[:, :, :16] = -128 + 16 * np.arange(16)
    ctx[:, :, 16] = 127
    return model_of(np.full((R, QT, S2), 95, dtype=np.int64), ctx)


def negative_cycle_probe(R, S2):
    """Cycle entries -128 + (col + q + r) mod 32, all negative; context entries 95 + ctx, all large: bytes 0 .. 47."""
    r, q, col = _grid(R, S2)
    ctx = np.broadcast_to(95 + np.arange(D, dtype=np.int64), (R, QT, D))
    return model_of(-128 + (col + q + r) % 32, ctx)


def row_probe(R, S2, m):
    """One entry per model row, -128 + (37 r + q) mod m against the constant context 95: output byte (37 r + q) mod m, no
    cycle or context variation.  R x 43 rows are more than 256 bytes: two moduli (251, 239) name the row together."""
    r, q, col = _grid(R, S2)
    cyc = np.broadcast_to(-128 + (37 * r + q) % m, (R, QT, S2))
    return model_of(cyc, np.full((R, QT, D), 95, dtype=np.int64))


PROBES = ('col161', 'col157', 'context', 'negcycle', 'row251', 'row239')


def probe(name, R, S2):
    if name.startswith('col'):
        return column_probe(R, S2, int(name[3:]))
    if name.startswith('row'):
        return row_probe(R, S2, int(name[3:]))
    return {'context': context_probe, 'negcycle': negative_cycle_probe}[name](R, S2)


def probes(R, S2):
    return {name: probe(name, R, S2) for name in PROBES}


def _bump(model, r, q, col, by):
    meanq, rgdq, qdq, posdq, dinucdq = model
    posdq = posdq.copy()
    posdq[r, q, col] += by
    return meanq, rgdq, qdq, posdq, dinucdq


def one_past_low(R, S2, r, q, col):
    """The context probe with the cycle entry of (r, q, col) at 94: with context AA (-128) that base sums to -1."""
    return _bump(context_probe(R, S2), r, q, col, -1)


def one_past_high(R, S2, r, q, col):
    """... at 96: with no context (127) that base sums to 256."""
    return _bump(context_probe(R, S2), r, q, col, +1)


ONE_PAST_CTX = {'low': 0, 'high': D - 1}             # the context a base must have to leave the range under each


def int8_misfit(R, S2):
    """Cycle entries 200, context entries -100: no entry fits int8, every sum is 133."""
    return model_of(np.full((R, QT, S2), 200, dtype=np.int64), np.full((R, QT, D), -100, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------- reads
def group_of(npairs, R):
    """Read group of pair k: uneven shares -- one group owns 12 pairs of 20 (enough workgroups of its own for the XCD
    remap on grouped rows), and with 8 groups group 5 is empty."""
    if R == 1:
        return np.zeros(npairs, dtype=np.uint32)
    pattern = np.array([0, 3, 1, 3, 3, 1, 3, 2, 3, 3, 4, 3, 6, 3, 3, 6, 3, 7, 3, 3], dtype=np.int64)
    if R < 8:                                                        # the large share goes to the last group
        pattern = np.where(pattern == 3, R - 1, pattern % (R - 1))
    return pattern.astype(np.uint32)[np.arange(npairs) % len(pattern)]


def reads(S, R, n, seed, pitch=None, len_lo=None, single_end=False, S2=None, pair_pitch=None):
    """n reads (n even) of S bases as host planes (seq, cseq, qual, meta), mates alternating and sharing a read group:
    qualities uniform over 33 .. 75; in the first two reads and in every 37th pair a ramp over every byte 0 .. 75; bases
    ACGT with 5 % N, N as the last base of some mates and on both sides of every 256th chunk (a wave's first chunk and
    the base before it), of rows of `pitch` bytes and of mate-pair rows; cseq differs from seq in 4 % of the bases.
    (Byte 76, quality 43, has no model row: the reference raises IndexError for the whole batch, so a test that wants
    it plants it in a copy.)
    len_lo: half of the reads get a length in [len_lo, S] (one read per row only).  single_end: nobody is second.
    Asserts that every quality 6 .. 42, all 17 contexts and every column a read of S bases can reach under S2 columns
    occur on counted bases."""
    assert n % 2 == 0
    S2 = S2 or 2 * S
    pitch = pitch or (S + 15) // 16 * 16
    rng = np.random.default_rng(seed)
    lens = np.full(n, S, dtype=np.int64)
    if len_lo is not None:
        short = rng.random(n) < 0.5
        lens[short] = rng.integers(len_lo, S + 1, size=int(short.sum()))
        lens[:2] = S
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=(n, pitch))]
    seq[rng.random((n, pitch)) < 0.05] = ord('N')
    qual = rng.integers(33, 33 + QT, size=(n, pitch)).astype(np.uint8)
    ramp = np.arange(33 + QT, dtype=np.int64)
    for k, r in enumerate([0, 1] + list(range(2 * 37, n, 2 * 37)) + list(range(2 * 37 + 1, n, 2 * 37))):
        qual[r] = ramp[(np.arange(pitch) + 38 * k) % len(ramp)]
    last = lens - 1
    seq[np.arange(0, n, 11), last[0:n:11]] = ord('N')
    seq[np.arange(1, n, 13), last[1:n:13]] = ord('N')
    for c in range(256, n * (pitch // 16), 256):                     # one read per row
        for byte in (16 * c - 1, 16 * c):
            row, p = divmod(byte, pitch)
            seq[row, p] = ord('N')
    pp = pair_pitch or (2 * S + 1 + 15) // 16 * 16
    for c in range(256, (n // 2) * (pp // 16), 256):                 # mate-pair rows: [mate 1][separator][mate 2]
        for byte in (16 * c - 1, 16 * c):
            row, p = divmod(byte, pp)
            if p < S:
                seq[2 * row, p] = ord('N')
            elif S < p <= 2 * S:
                seq[2 * row + 1, p - S - 1] = ord('N')
    cseq = seq.copy()
    wrong = (rng.random((n, pitch)) < 0.04) & (seq != ord('N'))
    cseq[wrong] = np.frombuffer(b'ACGT', dtype=np.uint8)[(_CODE[seq[wrong]] + 1) % 4]
    beyond = np.arange(pitch)[None, :] >= lens[:, None]              # the layout contract: N and 0 behind the read
    seq[beyond] = cseq[beyond] = ord('N')
    qual[beyond] = 0
    second = np.zeros(n, dtype=np.uint32) if single_end else (np.arange(n, dtype=np.uint32) & np.uint32(1))
    rg = np.repeat(group_of(n // 2, R), 2)
    meta = (lens.astype(np.uint32) | (rg << np.uint32(16)) | (second << np.uint32(31))).astype(np.uint32)
    if n >= 400:
        L = lookups(seq, qual, meta, S2)
        assert np.array_equal(np.unique(L.q), np.arange(MINSCORE, QT))
        assert np.array_equal(np.unique(L.ctx), np.arange(D))
        want = np.arange(S) if single_end else np.concatenate([np.arange(S), np.arange(S2 - S, S2)])
        assert np.array_equal(np.unique(L.col), np.unique(want))
        assert set(np.unique(L.r).tolist()) == set(np.unique(rg).tolist())
        assert (qual[:2, :S] < 33).any() and (qual[:2, :S] == 32 + QT).any()
    return seq, cseq, qual, meta


# ---------------------------------------------------------------------------------------------------- mistakes
def _column_plus_one(L, R):
    return L.r, L.q, (L.col + 1) % L.S2, L.ctx


def _mirror_dropped(L, R):
    return L.r, L.q, np.where(L.second == 1, L.pos, L.col), L.ctx


def _context_transposed(L, R):
    return L.r, L.q, L.col, np.where(L.ctx < 16, 4 * (L.ctx % 4) + L.ctx // 4, L.ctx)


def _no_context(L, R):
    return L.r, L.q, L.col, np.full_like(L.ctx, D - 1)


def _quality_plus_one(L, R):
    return L.r, (L.q + 1) % QT, L.col, L.ctx


def _group_plus_one(L, R):
    return (L.r + 1) % R, L.q, L.col, L.ctx


# what a kernel could get wrong about the indices: name -> (r, q, col, ctx) it would look up instead.  The twins mapping
# (k3_fill_pair_lut: a row's second half reads the forward columns) in place of the mirror IS the dropped mirror, seen
# from the pair LUT; both names are kept because they are different lines of the product.
MISTAKES = {
    'column + 1': _column_plus_one,
    'mirror dropped': _mirror_dropped,
    'twins mapping for the mirror': _mirror_dropped,
    'context transposed': _context_transposed,
    'no context': _no_context,
    'quality row + 1': _quality_plus_one,
    'read group + 1': _group_plus_one,
}
