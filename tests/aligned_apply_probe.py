"""
Probe models, rows and a plain reference for ApplyBQSR on aligned rows (kaa_apply, csrc/kbbq_apply_aligned.h): no GPU, no
product code, no oracle.  The pattern is tests/k2_probe.py's: models whose OUTPUT BYTE names the index that was looked up,
entries on the ends of what the model forms hold, and rows that reach every piece of the kernel's geometry.

    analyse / reference_apply   the rule of include/kbbq_hip.h ("ApplyBQSR on aligned rows") in NumPy, on host planes
    f64_rows                    the KBBQ_ALIGNED_F64 blob of a model, stated from the header
    int_probes, int16_ends      integer models: k2_probe's (any R, S2), generic ones for other Qt, the ends of int16
    near_probe, order_probe     float models: levels next to integers, and cells whose truncated sum depends on the order
    float_cell                  a flat float model with one cell of a chosen total (the edges of the byte range, +-2e9)
    SHAPES, rows                host planes for the shapes of tests/test_gpu_aligned_apply_probe.py
    MISTAKES                    index mistakes a kernel could make, each as a variant of the reference
    coverage                    what the rows of a shape reach, computed from the reference alone

A model is (meanq [R], rgdq [R], qdq [R, Qt], posdq [R, Qt, S2], dinucdq [R, Qt, 17]), integer or float64.

The rule.  A row's meta word: bits 0..15 length L, 16..27 read group, 28 the SOURCE qualities are the OQ plane (else QUAL),
29 the CONTEXT qualities are the OQ plane, 30 reverse strand, 31 second mate.  In SEQUENCING orientation (a reverse row
flipped and complemented, everything but ACGT becoming N) base j has source quality q and context quality c; with q <
minscore it keeps its source byte; otherwise its new byte is 33 + meanq + rgdq + qdq[q] + dinucdq[q][ctx] + posdq[q][col],
col = j (first mate) or S2 - 1 - j (second), ctx = 4 code(prev) + code(cur) (A0 T1 G2 C3) when j >= 1, c >= 6 and neither base
is N, else 16.  Errors, with the row: TypeError for a forward row with a letter outside ACGTN in a dinucleotide that is looked
up (c >= 6, j >= 1, neither base N -- whatever the base's SOURCE quality: the reference computes the covariate for the whole
read); IndexError for q >= Qt or j >= S2 on a base with q >= minscore; RangeError for a byte outside 0..255.  The first
offending row decides; within a row Type, then Index, then Range (kbbq_ctx_status).
"""
import numpy as np

import k2_probe as K

D = 17
CTX_MINSCORE = 6                     # the context's threshold is fixed, whatever `minscore` says
WAVE = 64                            # chunks (lanes) per wave
A, C, G, T, N_ = (ord(x) for x in 'ACGTN')

_CODE = np.full(256, -1, dtype=np.int64)                 # A0 T1 G2 C3, N 4, anything else -1
for _k, _c in enumerate('ATGCN'):
    _CODE[ord(_c)] = _k
_COMP = np.full(256, N_, dtype=np.uint8)                 # Dinucleotide.complement.get(x, 'N')
for _a, _b in ('AT', 'TA', 'CG', 'GC'):
    _COMP[ord(_a)] = ord(_b)
_KEEP = np.full(256, N_, dtype=np.uint8)                 # (the mistake "complement dropped": ACGT as they are)
for _a in 'ACGT':
    _KEEP[ord(_a)] = ord(_a)
_LETTER_OF = np.array([A, T, G, C], dtype=np.uint8)


class RangeError(ValueError):
    """A new byte outside 0..255 (KBBQ_E_RANGE)."""


class Analysis:
    """What the rule does with a batch; every array is [n, pitch] in ALIGNED orientation unless said otherwise."""


# ---------------------------------------------------------------------------------------------------- reference
def _fields(meta):
    meta = np.asarray(meta).astype(np.int64)
    return (meta & 0xFFFF, (meta >> 16) & 0xFFF, (meta >> 28) & 1, (meta >> 29) & 1, (meta >> 30) & 1, (meta >> 31) & 1)


def lookups(seq, qual, oq, meta, S2, minscore=6, wrong=None):
    """The indices every base of a batch looks up, in SEQUENCING orientation ([n, pitch], index j): `ai` the aligned
    position of base j, `inside`, `looked` (source quality >= minscore), `r`, `q`, `col`, `ctx`, `cq`, `pair` (an ACGT
    dinucleotide at j >= 1, whatever its quality), `type_bad` (a looked-up dinucleotide with a letter outside ACGTN), `jj`
    (the cycle).  wrong: a name of MISTAKES -- what a kernel with that mistake would look up instead."""
    seq = np.asarray(seq)
    qual = np.asarray(oq if qual is None else qual)
    oq = np.asarray(qual if oq is None else oq)
    n, pitch = seq.shape
    L, rg, src_oq, ctx_oq, rev, second = _fields(meta)
    j = np.broadcast_to(np.arange(pitch, dtype=np.int64)[None, :], (n, pitch))
    inside = j < L[:, None]
    revc = np.broadcast_to(rev[:, None] == 1, (n, pitch))
    ai = np.where(inside, np.where(revc, L[:, None] - 1 - j, j), 0)
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], (n, pitch))
    src = np.where(src_oq[:, None] == 1, oq, qual)
    cpl = np.where(ctx_oq[:, None] == 1, oq, qual)
    if wrong == 'context quality from the source plane':
        cpl = src
    if wrong == 'source from the context plane':
        src = cpl
    src_b = src[rows, ai].astype(np.int64)
    sq = src_b - 33
    cq = cpl[rows, ai].astype(np.int64) - 33
    s = seq[rows, ai]
    comp = _KEEP if wrong == 'complement dropped' else _COMP
    s = np.where(revc, comp[s], s)
    cur = np.where(inside, _CODE[s], 4)
    prev = np.full_like(cur, 4)
    prev[:, 1:] = cur[:, :-1]
    if wrong == 'reverse neighbour from i - 1':              # i - 1 is j + 1
        nxt = np.full_like(cur, 4)
        nxt[:, :-1] = cur[:, 1:]
        prev = np.where(revc, nxt, prev)
    first = (j >= 1)
    # where the neighbour lies in the aligned plane: i - 1 (forward) or i + 1 (reverse)
    nai = np.where(revc, ai + 1, ai - 1)
    if wrong == 'chunk edge: no neighbour':
        prev = np.where(nai // 16 != ai // 16, 4, prev)
    if wrong == 'wave edge: no neighbour':
        cpr = pitch // 16
        chunk, nchunk = rows * cpr + ai // 16, rows * cpr + nai // 16
        prev = np.where(chunk // WAVE != nchunk // WAVE, 4, prev)
    if wrong in ('first base takes the row before', 'last base takes the row after'):
        # j = 0 of a forward row reads the byte before the row, of a reverse row the byte after its last base
        flat = np.concatenate([[0], seq.reshape(-1), [0]]).astype(np.uint8)
        which = ~revc if wrong == 'first base takes the row before' else revc
        at = rows * pitch + nai + 1
        nb = flat[np.clip(at, 0, flat.size - 1)]
        nb = np.where(revc, _COMP[nb], _KEEP[nb])
        take = which & (j == 0) & inside
        prev = np.where(take, _CODE[nb], prev)
        first = first | take
    thr = {'context threshold 5': 5, 'context threshold 7': 7, 'context threshold is minscore': minscore}.get(wrong, CTX_MINSCORE)
    has = first & inside & (cq >= thr) & (cur != 4) & (prev != 4)
    type_bad = has & ((cur < 0) | (prev < 0))
    ok = has & ~type_bad
    a, b = (cur, prev) if wrong == 'prev / cur transposed' else (prev, cur)
    ctx = np.where(ok, 4 * a + b, D - 1)
    jj = ai if wrong == 'strand flip of the cycle dropped' else j
    col = np.where((second[:, None] == 1) & (wrong != 'mirror of read 2 dropped'), S2 - 1 - jj, jj)
    r = np.broadcast_to(rg[:, None], (n, pitch))
    q = sq
    X = Analysis()
    X.n, X.pitch, X.S2, X.minscore = n, pitch, S2, minscore
    X.L, X.rev, X.second, X.rows = L, rev, second, rows
    X.ai, X.inside, X.looked = ai, inside, inside & (sq >= minscore)
    X.src_b, X.r, X.q, X.cq, X.col, X.ctx, X.jj = src_b, r, q, cq, col, ctx, jj
    X.pair = first & inside & (cur >= 0) & (cur < 4) & (prev >= 0) & (prev < 4)
    X.type_bad = type_bad
    X.wrong = wrong
    return X


def _sum(model, mode, r, q, col, ctx, wrong=None):
    """(values, out_of_range) of the model's cells: int64 sums, or the prescribed float64 sum truncated toward zero."""
    meanq, rgdq, qdq, posdq, dndq = (np.asarray(x) for x in model)
    if mode == 'lut':
        m = [x.astype(np.int64) for x in (meanq, rgdq, qdq, posdq, dndq)]
        assert all(np.array_equal(a, b) for a, b in zip(m, (meanq, rgdq, qdq, posdq, dndq))), 'LUT mode sums integers'
        v = m[0][r] + m[1][r] + m[2][r, q] + m[4][r, q, ctx] + m[3][r, q, col]
        return v, np.zeros(v.shape, dtype=bool)
    assert mode == 'f64'
    m = [x.astype(np.float64) for x in (meanq, rgdq, qdq, posdq, dndq)]
    base = (m[0][r] + m[1][r]) + m[2][r, q]
    dn, pos = m[4][r, q, ctx], m[3][r, q, col]
    if wrong == 'F64: base + (dinuc + pos)':
        s = base + (dn + pos)
    elif wrong == 'F64: (base + pos) + dinuc':
        s = (base + pos) + dn
    else:
        s = (base + dn) + pos
    far = ~(np.abs(s) < 1.0e9)
    s = np.where(far, 0.0, s)
    v = (np.floor(s) if wrong == 'F64: floor' else np.trunc(s)).astype(np.int64)
    return v, far


def analyse(seq, qual, oq, meta, model, minscore=6, mode='lut', wrong=None):
    """`lookups` and what comes of them: X.out (int64 bytes in ALIGNED orientation, not clamped, 0 at and beyond L), per row
    X.row_type / X.row_index / X.row_range, and X.error = (class, row) of the first offending row or None."""
    R, Qt, S2 = np.asarray(model[3]).shape
    X = lookups(seq, qual, oq, meta, S2, minscore, wrong)
    r, q, col = X.r, X.q, X.col
    if wrong == 'column + 1':
        col = (col + 1) % S2
    if wrong == 'quality row + 1':
        q = (q + 1) % Qt
    if wrong == 'read group + 1':
        r = (r + 1) % R
    if wrong == 'read group masked to 11 bits':
        r = r & 0x7FF
    index_bad = X.looked & ((q >= Qt) | (X.jj >= S2) | (r >= R))
    use = X.looked & ~index_bad
    v, far = _sum(model, mode, r[use], q[use], col[use], X.ctx[use], wrong)
    byte = v + 33
    range_bad = np.zeros_like(use)
    range_bad[use] = far | (byte < 0) | (byte > 255)
    new = np.where(X.inside, X.src_b, 0)
    new[use] = np.where(far, 1 << 30, byte)
    new[index_bad] = 0
    out = np.zeros((X.n, X.pitch), dtype=np.int64)
    out[X.rows[X.inside], X.ai[X.inside]] = new[X.inside]
    X.out, X.use = out, use
    X.row_type, X.row_index, X.row_range = X.type_bad.any(axis=1), index_bad.any(axis=1), range_bad.any(axis=1)
    X.error = None
    bad = np.flatnonzero(X.row_type | X.row_index | X.row_range)
    if len(bad):
        k = int(bad[0])
        X.error = (TypeError if X.row_type[k] else IndexError if X.row_index[k] else RangeError, k)
    return X


def aligned(X, plane):
    """A per-base array of an Analysis (sequencing orientation) as an ALIGNED plane; False / 0 at and beyond L."""
    out = np.zeros((X.n, X.pitch), dtype=plane.dtype)
    out[X.rows[X.inside], X.ai[X.inside]] = plane[X.inside]
    return out


def reference_apply(seq, qual, oq, meta, model, minscore=6, mode='lut'):
    """The new quality BYTES [n, pitch] (int64, not clamped); raises the error the header prescribes, with `.row`."""
    X = analyse(seq, qual, oq, meta, model, minscore, mode)
    if X.error is not None:
        exc = X.error[0]('row %d' % X.error[1])
        exc.row = X.error[1]
        raise exc
    return X.out


def f64_rows(model):
    """The KBBQ_ALIGNED_F64 blob as float64 [R, Qt, 18 + S2]: [(meanq + rgdq) + qdq, dinucdq[0..16], posdq[0..S2-1]]."""
    meanq, rgdq, qdq, posdq, dndq = (np.asarray(x).astype(np.float64) for x in model)
    base = (meanq + rgdq)[:, None] + qdq
    return np.ascontiguousarray(np.concatenate([base[..., None], dndq, posdq], axis=-1))


# ---------------------------------------------------------------------------------------------------- integer models
def _grid(R, Qt, S2):
    return (np.arange(R, dtype=np.int64)[:, None, None], np.arange(Qt, dtype=np.int64)[None, :, None],
            np.arange(S2, dtype=np.int64)[None, None, :])


def _context_entries(R, Qt):
    ctx = np.empty((R, Qt, D), dtype=np.int64)
    ctx[:, :, :16] = -128 + 16 * np.arange(16)
    ctx[:, :, 16] = 127
    return ctx


def int_probes(R, S2, Qt=K.QT):
    """name -> model.  Qt = 43: k2_probe.probes.  Any other Qt: the same constructions with Qt quality rows."""
    if Qt == K.QT:
        return K.probes(R, S2)
    r, q, col = _grid(R, Qt, S2)
    zero, flat = np.zeros((R, Qt, D), dtype=np.int64), np.full((R, Qt, D), 95, dtype=np.int64)
    made = {}
    for m in (161, 157):
        made['col%d' % m] = K.model_of((col + 5 * q + 17 * r) % m - 33, zero)
    made['context'] = K.model_of(np.full((R, Qt, S2), 95, dtype=np.int64), _context_entries(R, Qt))
    made['negcycle'] = K.model_of(-128 + (col + q + r) % 32, np.broadcast_to(95 + np.arange(D, dtype=np.int64), (R, Qt, D)))
    for m in (251, 239):
        made['row%d' % m] = K.model_of(np.broadcast_to(-128 + (37 * r + q) % m, (R, Qt, S2)), flat)
    return made


def one_past(R, S2, r, q, col, end, Qt=K.QT):
    """The context probe with the cycle entry of (r, q, col) moved by one: with context AA that base sums to -1 (end
    'low'), with no context to 256 ('high')."""
    meanq, rgdq, qdq, posdq, dndq = int_probes(R, S2, Qt)['context']
    posdq = posdq.copy()
    posdq[r, q, col] += -1 if end == 'low' else 1
    return meanq, rgdq, qdq, posdq, dndq


def int16_ends(R, S2, sign, Qt=K.QT):
    """Cycle entries sign * 32000 + (col + 5 q + 17 r) mod 208, context entries -sign * 32000 - 33 + 3 ctx (no context:
    48): every entry sits on an end of int16 and every sum + 33 lies in 0 .. 255, both ends included."""
    r, q, col = _grid(R, Qt, S2)
    ctx = np.broadcast_to(-sign * 32000 - 33 + 3 * np.arange(D, dtype=np.int64), (R, Qt, D))
    return K.model_of(sign * 32000 + (col + 5 * q + 17 * r) % 208, ctx)


INT16_ENDS = {'int16 +-': 1, 'int16 -+': -1}


# ---------------------------------------------------------------------------------------------------- float models
def near_probe(R, S2, Qt=K.QT):
    """Integer parts that name the index -- cycle part (col + 5 q + 17 r) mod 161 - 30, on every third quality row
    (...) mod 29 - 31: below zero, where truncation and floor part; dinucleotide part ctx mod 4 - 1 -- with every level a few
    units of 2^-46 off its integer: the exact sum lies next to an integer, on either side of it.  Bytes 1 .. 165."""
    r, q, col = _grid(R, Qt, S2)
    x = col + 5 * q + 17 * r
    cyc = np.where(q % 3 == 2, x % 29 - 31, x % 161 - 30)
    meanq, rgdq, qdq, posdq, dndq = K.model_of(cyc, np.zeros((R, Qt, D), dtype=np.int64))
    e = 2.0 ** -46
    meanq = meanq + e * ((np.arange(R) % 5) - 2)
    rgdq = rgdq + e * ((np.arange(R) % 3) - 1)
    qdq = qdq + e * ((np.arange(Qt)[None, :] * 7 + np.arange(R)[:, None]) % 9 - 4)
    posdq = posdq + e * ((col * 5 + q) % 11 - 5)
    dndq = (np.arange(D) % 4 - 1) + e * ((np.arange(D) * 3 + q) % 7 - 3) + np.zeros((R, 1, 1))
    return meanq, rgdq, qdq, posdq, dndq


_H = 2.0 ** -49                      # half a unit in the last place of a double in [16, 32)


ORDER_EVEN = (np.arange(D) % 2 == 0) & (np.arange(D) < 16)          # the contexts of order_probe's first kind


def order_probe(R, S2, Qt=K.QT):
    """Integer levels base = 17 + (q + r) mod 13 (exact in any order), every fifth quality row 50 lower; the dinucleotide entry
    just under 1 (even dinucleotides: 1 - 2^-53; odd ones and no context: 1 - 2^-49 - 2^-53) and the cycle entry -2^-49 (columns that
    are no multiple of 3: "minus") or +2^-49 ("plus").  For base in [16, 31), "odd" including no context:
        even ctx, minus col  (base + dn) + pos = base + 1 (a tie, to even)    base + (dn + pos) = base + 1 - 2^-48: truncates lower
        odd ctx,  plus col   (base + dn) + pos = base + 1 (a tie, to even)    (base + pos) + dn = base + 1 - 2^-48: truncates lower
    so a third and a sixth of the dinucleotide cells tell each of the two other association orders from the prescribed one."""
    r, q, col = _grid(R, Qt, S2)
    base = 17 + (np.arange(Qt)[None, :] + np.arange(R)[:, None]) % 13 - 50 * (np.arange(Qt)[None, :] % 5 == 4)
    meanq = (12 + np.arange(R) % 3).astype(np.float64)
    rgdq = (2 - np.arange(R) % 2).astype(np.float64)
    qdq = base - (meanq + rgdq)[:, None]
    dn = np.where(ORDER_EVEN, 1 - 2.0 ** -53, 1 - _H - 2.0 ** -53)
    dndq = np.broadcast_to(dn, (R, Qt, D)).copy()
    posdq = np.broadcast_to(np.where(col % 3 != 0, -_H, _H), (R, Qt, S2)).copy()
    return meanq, rgdq, qdq, posdq, dndq


def float_probes(R, S2, Qt=K.QT):
    return {'near': near_probe(R, S2, Qt), 'order': order_probe(R, S2, Qt)}


def float_cell(R, S2, r, q, col, total, Qt=K.QT):
    """A flat float model, every sum 20.5 (byte 53), whose cell (r, q, col) sums to `total` with any context."""
    meanq = np.full(R, 18.25)
    rgdq = np.full(R, 1.0)
    qdq = np.full((R, Qt), 0.75)
    posdq = np.full((R, Qt, S2), 0.25)
    dndq = np.full((R, Qt, D), 0.25)
    posdq[r, q, col] = total - 20.25
    assert ((meanq[r] + rgdq[r]) + qdq[r, q] + dndq[r, q, 0]) + posdq[r, q, col] == total
    return meanq, rgdq, qdq, posdq, dndq


def models(key, S2):
    """The models the GPU test runs on shape `key` under S2 columns: a list of (name, model, mode, blob) -- blob '_model':
    the product's applybqsr._model makes the kernel's blob (and must choose `mode`); blob 'rows': `f64_rows` does, for an
    integer model in F64 mode, which _model would always fold into the LUT.  The discriminating-power test certifies
    exactly this list."""
    s = SHAPES[key]
    made = []
    if key == 'long':
        ints = int_probes(1, S2)
        made += [(name, ints[name], 'lut', '_model') for name in ('col161', 'col157', 'context')]
        # 96 quality rows are more than the LUT form takes: _model hands an integer model to the float64 rows as it is
        made.append(('col161 of 96 rows', int_probes(1, S2, Qt=96)['col161'], 'f64', '_model'))
        made += [(name + ' of 96 rows', m, 'f64', '_model') for name, m in float_probes(1, S2, Qt=96).items()]
        return made
    if key == 'rg4096':
        ints = int_probes(s.R, S2)
        made += [(name, ints[name], 'lut', '_model') for name in ('row251', 'row239', 'col161', 'context')]
        made += [(name, m, 'f64', '_model') for name, m in float_probes(s.R, S2).items()]
        return made
    if key in ('qt95', 'qt223'):
        mode = 'lut' if key == 'qt95' else 'f64'
        made += [(name, m, mode, '_model') for name, m in int_probes(s.R, S2, s.Qt).items()]
        if key == 'qt223':
            made += [(name, m, 'f64', '_model') for name, m in float_probes(s.R, S2, s.Qt).items()]
        return made
    ints = int_probes(s.R, S2)
    made += [(name, m, 'lut', '_model') for name, m in ints.items()]
    made += [(name, int16_ends(s.R, S2, sign), 'lut', '_model') for name, sign in INT16_ENDS.items()]
    made += [(name + ' as float64 rows', ints[name], 'f64', 'rows') for name in ('col161', 'context', 'row251')]
    made += [(name, m, 'f64', '_model') for name, m in float_probes(s.R, S2).items()]
    return made


def order_model(key, S2):
    """The order-sensitive float rows as `models` hands them to shape `key`."""
    s = SHAPES[key]
    return order_probe(s.R, S2, 96 if key == 'long' else s.Qt)


def runs_order_probe(key):
    """Whether the model list of shape `key` holds the order-sensitive float rows."""
    return any(name.startswith('order') for name, _, _, _ in models(key, 16))


# ---------------------------------------------------------------------------------------------------- rows
class Shape:
    pass


def _shape(n, pitch, lengths, S2s, R=3, Qt=K.QT, minscores=(6,), groups=None, strands=None, what=''):
    s = Shape()
    s.n, s.pitch, s.lengths, s.S2s, s.R, s.Qt, s.minscores, s.groups, s.strands, s.what = (
        n, pitch, lengths, S2s, R, Qt, minscores, groups, strands, what)
    return s


# strands: (reverse, second) per row where the shape fixes them; lengths: cycled over the rows in a fixed shuffle
SHAPES = {
    'p16': _shape(257, 16, [16, 0, 16, 16, 1, 15, 16, 7, 16, 0, 2, 16, 16, 9, 3, 16], [32],
                  what='one chunk a row; 257 chunks: a full workgroup and one with ONE live lane'),
    'p48': _shape(200, 48, [48, 1, 15, 16, 48, 17, 31, 32, 48, 33, 47, 48], [96],
                  what='3 chunks a row: rows straddle wave and workgroup edges at every phase'),
    'p160': _shape(103, 160, [150, 151, 160], [300, 302, 320], what='the everyday shape'),
    'p1040': _shape(9, 1040, [1040, 1040, 1025, 1040, 1040, 1025, 1040, 1040, 1040], [2080],
                    what="65 chunks a row: every wave's lane 0 and lane 63 sit mid-row"),
    'long': _shape(3, 65536, [65535, 65521, 4097], [65536], R=1, strands=[(0, 1), (1, 0), (1, 1)],
                   what='columns beyond 32767, read 2 mirrored from the far end'),
    'rg4096': _shape(64, 32, [16, 32, 9, 16, 32, 16, 16, 32], [16], R=4096, groups=[0, 1, 2047, 2048, 4095],
                     what='12-bit read groups; bases at j >= S2 stay below minscore'),
    'qt95': _shape(64, 48, [48, 33, 48, 17, 48, 40], [96], R=2, Qt=95, minscores=(0, 2, 20), what='LUT, bytes up to 127'),
    'qt223': _shape(64, 48, [48, 33, 48, 17, 48, 40], [96], R=2, Qt=223, minscores=(0, 2, 20),
                    what='F64, bytes up to 255: unsigned handling'),
}


def _target(c):
    """The byte (0 or 15) of chunk c at which `rows` plants a context, or None; no two planted pairs overlap."""
    lane, wave = c % WAVE, c // WAVE
    if lane == 0:
        return 0 if wave % 2 == 0 else 15
    if lane == WAVE - 1:
        return 15 if wave % 2 == 0 else 0
    return (0, 15, None)[lane % 3]


def rows(key, seed=0):
    """Host planes (seq, qual, oq, meta) of shape `key`.  Strand x mate and the two plane bits are mixed row by row (all 16
    combinations, shuffled); qual and oq are different planes with different bytes; letters ACGT with 8 % N.  Both
    quality planes are drawn alike -- which one is a row's source and which its context plane is the row's bits alone: 45 %
    of the bytes within 2 of one of the shape's minscores or of the context's 6, the rest uniform over the model's rows.  On top of the random letters two chunks of three carry a PLANTED dinucleotide at its
    byte 0 or byte 15 (`_target`), the 17 contexts in turn per (strand, byte, lane 0 / lane 63 / another lane), with both
    planes' qualities at that base high enough to be looked up -- so that which contexts cross a chunk or wave edge does not
    hang on the seed.  Bytes at and beyond L are 0 in every plane."""
    s = SHAPES[key]
    rng = np.random.default_rng([seed, sum(key.encode())])
    n, pitch = s.n, s.pitch
    L = np.array([s.lengths[k % len(s.lengths)] for k in range(n)], dtype=np.int64)
    combo = np.concatenate([rng.permutation(16) for _ in range((n + 15) // 16)])[:n]
    rev, second, src_oq, ctx_oq = combo & 1, (combo >> 1) & 1, (combo >> 2) & 1, (combo >> 3) & 1
    if s.strands is not None:
        rev, second = (np.array(x, dtype=np.int64) for x in zip(*s.strands))
    if s.groups is not None:
        rg = np.array(s.groups, dtype=np.int64)[np.arange(n) % len(s.groups)]
    else:
        rg = rng.integers(0, s.R, size=n)
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, size=(n, pitch))].copy()
    seq[rng.random((n, pitch)) < 0.08] = N_

    def quality(near, share):
        q = rng.integers(0, s.Qt, size=(n, pitch))
        pick = rng.random((n, pitch)) < share
        centre = np.array(near, dtype=np.int64)[rng.integers(0, len(near), size=(n, pitch))]
        return np.where(pick, np.clip(centre + rng.integers(-2, 2, size=(n, pitch)), 0, s.Qt - 1), q)
    planes = [quality(list(s.minscores) + [CTX_MINSCORE], 0.45) for _ in range(2)]
    qual, oq = ((33 + p).astype(np.uint8) for p in planes)
    same = qual == oq
    oq[same] = 33 + (oq[same].astype(np.int64) - 33 + 1) % s.Qt          # different bytes everywhere
    # bases at j >= S2 are not looked up: their source quality stays below every minscore of the shape
    S2 = min(s.S2s)
    if (L > S2).any():
        assert min(s.minscores) > 0
        i = np.arange(pitch)[None, :]
        j = np.where(rev[:, None] == 1, L[:, None] - 1 - i, i)
        low = (j >= S2) & (i < L[:, None])
        qual[low] = 33 + rng.integers(0, min(s.minscores), size=int(low.sum()))
        oq[low] = 33 + (qual[low].astype(np.int64) - 33 + 1) % min(s.minscores) if min(s.minscores) > 1 else qual[low]
    # the planted contexts
    turn = {}
    cpr = pitch // 16
    hi = 33 + min(max(s.minscores) + 5, s.Qt - 2)
    for c in range(n * cpr):
        b = _target(c)
        if b is None:
            continue
        row, k = divmod(c, cpr)
        i = 16 * k + b
        ni = i + 1 if rev[row] else i - 1
        j = L[row] - 1 - i if rev[row] else i
        if i >= L[row] or ni < 0 or ni >= L[row] or j >= S2:
            continue
        lane = c % WAVE
        slot = (int(rev[row]), b, lane if lane in (0, WAVE - 1) else -1)
        ctx = turn.get(slot, 0)
        turn[slot] = (ctx + 1) % D
        if ctx == D - 1:
            seq[row, ni] = N_
            seq[row, i] = _LETTER_OF[(c // 7) % 4]
        else:
            pair = _LETTER_OF[[ctx // 4, ctx % 4]]
            if rev[row]:
                pair = _COMP[pair]
            seq[row, ni], seq[row, i] = pair
        qual[row, i], oq[row, i] = hi, hi + 1
    beyond = np.arange(pitch)[None, :] >= L[:, None]
    seq[beyond] = 0
    qual[beyond] = 0
    oq[beyond] = 0
    meta = (L | (rg << 16) | (src_oq << 28) | (ctx_oq << 29) | (rev << 30) | (second << 31)).astype(np.uint32)
    return seq, qual, oq, meta


# ---------------------------------------------------------------------------------------------------- mistakes
# name -> the modes it exists in.  Each is a `wrong=` of lookups / analyse: the reference with that one line changed.
MISTAKES = {
    'strand flip of the cycle dropped': ('lut', 'f64'),
    'complement dropped': ('lut', 'f64'),
    'reverse neighbour from i - 1': ('lut', 'f64'),
    'prev / cur transposed': ('lut', 'f64'),
    'mirror of read 2 dropped': ('lut', 'f64'),
    'context quality from the source plane': ('lut', 'f64'),
    'source from the context plane': ('lut', 'f64'),
    'context threshold 5': ('lut', 'f64'),
    'context threshold 7': ('lut', 'f64'),
    'context threshold is minscore': ('lut', 'f64'),
    'chunk edge: no neighbour': ('lut', 'f64'),
    'wave edge: no neighbour': ('lut', 'f64'),
    'first base takes the row before': ('lut', 'f64'),
    'last base takes the row after': ('lut', 'f64'),
    'column + 1': ('lut', 'f64'),
    'quality row + 1': ('lut', 'f64'),
    'read group + 1': ('lut', 'f64'),
    'read group masked to 11 bits': ('lut', 'f64'),
    'F64: base + (dinuc + pos)': ('f64',),
    'F64: (base + pos) + dinuc': ('f64',),
    'F64: floor': ('f64',),
}

# (shape, mistake) pairs that cannot show, with the reason; every other pair must change a byte under some probe
_NO_RG = 'one read group: (0 + 1) mod 1 is 0'
_LOW_RG = 'read groups below 2048: the 11-bit mask changes nothing'
NOT_APPLICABLE = {
    ('p16', 'chunk edge: no neighbour'): 'one chunk a row: no neighbour lies in another chunk',
    ('p16', 'wave edge: no neighbour'): 'one chunk a row: no neighbour lies in another chunk',
    ('rg4096', 'wave edge: no neighbour'): '2 chunks a row divide the 64 of a wave: no row straddles a wave edge',
    ('long', 'first base takes the row before'): 'no row fills its pitch: the byte beside a row is padding',
    ('long', 'last base takes the row after'): 'no row fills its pitch: the byte beside a row is padding',
    ('long', 'read group + 1'): _NO_RG,
    ('rg4096', 'context threshold is minscore'): 'minscore is 6 in this shape',
    ('rg4096', 'chunk edge: no neighbour'): 'S2 = 16: the bases on either side of the one chunk edge are not both looked up',
}
for _w, _modes in MISTAKES.items():
    if _modes == ('f64',):
        NOT_APPLICABLE['qt95', _w] = 'the shape of the LUT form: 95 quality rows, no F64 run'
for _key, _s in SHAPES.items():
    if _key != 'rg4096':
        NOT_APPLICABLE[_key, 'read group masked to 11 bits'] = _LOW_RG
    if _s.minscores == (6,) and _key != 'rg4096':
        NOT_APPLICABLE[_key, 'context threshold is minscore'] = 'minscore is 6 in this shape'


# ---------------------------------------------------------------------------------------------------- coverage
def coverage(key, planes, S2, minscore):
    """What the looked-up bases of a shape's rows reach, from `lookups` alone: a dict of sets and counts."""
    seq, qual, oq, meta = planes
    X = lookups(seq, qual, oq, meta, S2, minscore)
    m = X.looked
    byte, chunk = X.ai % 16, X.rows * (X.pitch // 16) + X.ai // 16
    lane = chunk % WAVE
    rev = np.broadcast_to(X.rev[:, None], m.shape)
    second = np.broadcast_to(X.second[:, None], m.shape)
    cov = {}
    cov['contexts'] = {(int(a), int(b)) for a, b in zip(rev[m], X.ctx[m])}
    for b in (0, 15):
        at = m & (byte == b)
        cov['byte', b] = {(int(a), int(c)) for a, c in zip(rev[at], X.ctx[at])}
        for ln in (0, WAVE - 1):
            w = at & (lane == ln)
            cov['byte', b, 'lane', ln] = {(int(a), int(c)) for a, c in zip(rev[w], X.ctx[w])}
    cov['columns'] = {mate: set(np.unique(X.col[m & (second == mate)]).tolist()) for mate in (0, 1)}
    pair = X.pair & m
    cov['context quality on a pair'] = set(np.unique(X.cq[pair]).tolist())
    cov['source quality'] = set(np.unique(X.q[X.inside]).tolist())
    cov['looked up'] = int(m.sum())
    cov['strand x mate'] = {(int(a), int(b)) for a, b in zip(X.rev, X.second)}
    cov['planes'] = {int(x) for x in (np.asarray(meta).astype(np.int64) >> 28) & 3}
    return cov


def order_sensitive(planes, model, minscore=6):
    """Looked-up bases whose byte differs under each of the two other association orders: (n2, n3)."""
    seq, qual, oq, meta = planes
    right = analyse(seq, qual, oq, meta, model, minscore, 'f64')
    return tuple(int((analyse(seq, qual, oq, meta, model, minscore, 'f64', w).out != right.out).sum())
                 for w in ('F64: base + (dinuc + pos)', 'F64: (base + pos) + dinuc'))
