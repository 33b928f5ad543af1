"""
A NumPy statement of K1's tally (no product code, no oracle), the choice of K1 form the launch layer makes, restated, and the
hand-made reads the K1 route tests run on (tests/test_k1_tally_host.py, tests/test_gpu_k1_routes.py).

reference_tally() is recalibrate.py:57-119 of the reference as ONE vectorised pass over padded planes: every base of every
read at once, no running maximum of the read lengths (so rows may come in any order of length: the oracle refuses a read
shorter than one before it), the second-in-pair column 2 * len - 1 - pos of compare_reads.py as the device states
it.  k1_plan() restates accumulate_rows / k1_geometry / k1_lds_plan / kbbq_accumulate_band_dev (csrc/kbbq_hip.hip)
so that a test can assert, before anything runs, which kernel form and which LDS geometry its shape reaches.
"""
import numpy as np

NQ = 43                                                 # qualities 0..42
LETTERS = np.frombuffer(b'ACGTN', dtype=np.uint8)
# context = 4 * code(prev) + code(cur) with the codes of compare_reads.py:199 (A0 T1 G2 C3); 4: N, no context
_CODE = np.full(256, -1, dtype=np.int64)
for _c, _v in zip(b'ATGCN', range(5)):
    _CODE[_c] = _v

MISTAKES = ('mirror_off_by_one', 'mirror_with_S', 'first_base_context', 'prev_cur_swapped', 'N_is_a_context', 'gt_for_ge',
            'split_on_cycle', 'read_group_ignored', 'second_ignored', 'split_ignored')


def pair_pitch(S2):
    return (S2 + 1 + 15) // 16 * 16


def _tally(seq, cseq, qual, meta, R, S2, minscore, dinuc_minscore, pairs, twins, mistake):
    seq, cseq, qual = np.asarray(seq), np.asarray(cseq), np.asarray(qual)
    n, pitch = seq.shape
    assert cseq.shape == seq.shape == qual.shape and seq.dtype == cseq.dtype == qual.dtype == np.uint8
    assert mistake is None or mistake in MISTAKES
    m = np.asarray(meta).astype(np.int64) & 0xFFFFFFFF
    assert m.shape == (n,)
    length, rg, second = (m & 0xFFFF)[:, None], ((m >> 16) & 0x7FFF)[:, None], ((m >> 31) & 1)[:, None]
    dm = minscore if dinuc_minscore is None else dinuc_minscore
    S = S2 // 2
    at = np.arange(pitch, dtype=np.int64)[None, :]
    if pairs:
        # [mate 1: S][separator][mate 2: S][padding]; the byte offset in the row is the stored cycle index
        assert pitch == pair_pitch(S2) and np.all(length == 2 * S + 1) and not second.any()
        inside = np.broadcast_to((at < 2 * S + 1) & (at != S), (n, pitch))
        mate2 = at > S
        pos = np.where(mate2, at - S - 1, at)
        col = np.where(mate2 & (not twins), 2 * S - 1 - pos, pos)
        first = np.broadcast_to((at == 0) | (at == S + 1), (n, pitch))
        if mistake == 'mirror_off_by_one':
            col = np.where(mate2 & (not twins), 2 * S - 2 - pos, pos)
        if mistake == 'second_ignored':
            col = pos
        col = np.broadcast_to(col, (n, pitch))
    else:
        assert not twins
        assert np.all(length <= pitch)
        inside = at < length
        first = np.broadcast_to(at == 0, (n, pitch))
        mirror = 2 * length - 1 - at
        if mistake == 'mirror_off_by_one':
            mirror = 2 * length - 2 - at
        if mistake == 'mirror_with_S':
            mirror = 2 * S - 1 - at
        if mistake == 'second_ignored':
            second = np.zeros_like(second)
        col = np.where(second == 1, mirror, at)
    if mistake == 'read_group_ignored':
        rg = np.zeros_like(rg)
    code = _CODE[seq]
    # what is not modelled is refused: letters outside ACGTN (the reference's TypeError rule), qualities above 42 or below 0
    assert np.all(code[inside] >= 0) and np.all(_CODE[cseq][inside] >= 0), 'a letter outside ACGTN'
    q = qual.astype(np.int64) - 33
    assert np.all((q[inside] >= 0) & (q[inside] < NQ)), 'a quality outside 0..42'
    assert np.all(rg < R) and np.all(col[inside] >= 0) and np.all(col[inside] < S2)
    err = seq != cseq
    above = (lambda a, b: a > b) if mistake == 'gt_for_ge' else (lambda a, b: a >= b)
    if mistake == 'split_ignored':
        dm = minscore
    counted = inside & above(q, minscore)
    cyc_counted = counted & above(q, dm) if mistake == 'split_on_cycle' else counted
    prev = np.concatenate([np.full((n, 1), 4, dtype=np.int64), code[:, :-1]], axis=1)
    has_prev = ~first
    if mistake == 'first_base_context':
        has_prev, prev = np.ones_like(first), np.where(first, 0, prev)              # an 'A' in front of every read
    cur = code
    if mistake == 'N_is_a_context':
        prev, cur = np.where(prev == 4, 0, prev), np.where(cur == 4, 0, cur)
    ctx_counted = counted & above(q, dm) & has_prev & (prev < 4) & (cur < 4)
    ctx = 4 * cur + prev if mistake == 'prev_cur_swapped' else 4 * prev + cur

    rgq = np.broadcast_to(rg, (n, pitch)) * NQ + q

    def hist(where, index, width):
        flat = (rgq[where] * width + index[where])
        return np.bincount(flat, minlength=R * NQ * width).astype(np.int64).reshape(R, NQ, width)
    return (hist(cyc_counted & err, col, S2), hist(cyc_counted, col, S2), hist(ctx_counted & err, ctx, 16), hist(ctx_counted, ctx, 16))


def reference_tally(seq, cseq, qual, meta, R, S2, minscore, dinuc_minscore=None, pairs=False, twins=False):
    """(pos_errs [R, 43, S2], pos_total, dinuc_errs [R, 43, 16], dinuc_total) as int64 -- the shapes of Tables.to_host() -- of the
    reads in padded planes [n, pitch] with the sidecar words len | rg << 16 | second << 31.  pairs: the planes are mate-pair rows
    (pitch = roundup16(S2 + 1), sidecar word S2 + 1 | rg << 16); twins: both halves of such a row are first in pair.
    A base counts where quality >= minscore; into the context tables where also quality >= dinuc_minscore, it is not a read's
    first base and neither it nor the base before it is N.  Column: pos, or 2 * len - 1 - pos for a second-in-pair read."""
    return _tally(seq, cseq, qual, meta, R, S2, minscore, dinuc_minscore, pairs, twins, None)


def mistaken_tally(mistake, seq, cseq, qual, meta, R, S2, minscore, dinuc_minscore=None, pairs=False, twins=False):
    """reference_tally with ONE index mistake of MISTAKES (the discrimination test of tests/test_k1_tally_host.py)."""
    return _tally(seq, cseq, qual, meta, R, S2, minscore, dinuc_minscore, pairs, twins, mistake)


# ---- which form of K1 a shape reaches ---------------------------------------------------------------------------------------

THREADS, FLUSH_ITERS = 1024, 48                         # K1V3_THREADS, K1V3_FLUSH_ITERS
ROWS_PER_ITER = THREADS // 64 * 64                      # rows one workgroup walks per iteration: 16 waves x 64


def k1_plan(S, pitch, minscore, s_min, pairs=False, lds_bytes=163840, nib=False):
    """What accumulate_rows chooses for rows of `pitch` bytes whose longest read is S and whose shortest non-empty read is
    s_min (0: not promised).  route: 'v3' (k1v3_accumulate<., dn, ., 0>), 'joint' (its KJ = 19 / 13 instances: 4-bit mate-pair
    rows), 'plain' (k1_accumulate) or 'tiled' (k1_accumulate_tiled) -- the last two only serve character planes that are not
    grouped by read group, every other caller gets an error there.  attempt: 0 (16 copies, rows of 3S words), 1 (16 copies, rows
    trimmed by cut = s_min), 2 (8 copies and cut).  copy_bound: the most counts one 16-bit half of one copy of a context bin can
    receive per workgroup iteration; flush_rows: the rows a workgroup walks before its first flush."""
    cpr, nrows = pitch // 16, NQ + 1 - minscore
    if pairs:
        assert pitch == pair_pitch(2 * S)
    out = dict(route=None, attempt=None, dn=0, cut=0, ntrash=1, pos_copies=1, dn_flush_iters=0, lds=0, copy_bound=0, flush_rows=0)

    def done(**kw):
        out.update(kw)
        if out['dn']:
            out['copy_bound'] = THREADS // out['dn'] * 16 * cpr
            out['flush_rows'] = ROWS_PER_ITER * min(out['dn_flush_iters'], FLUSH_ITERS)
        return out
    if pairs and nib and cpr in (19, 13):
        row_bytes = (((16 * cpr + 31) & ~31) + 32 * 16) * 4
        for nt in ((1,) if cpr == 19 else (8, 4, 2, 1)):
            if (nrows - 1 + nt) * row_bytes <= lds_bytes:
                return done(route='joint', dn=16, ntrash=nt, dn_flush_iters=max(1, 65535 // (THREADS // 16 * 16 * cpr)),
                            lds=(nrows - 1 + nt) * row_bytes)
    trim = min(s_min, S) if (not pairs and s_min > 0) else 0
    for attempt in range(3 if trim else 1):
        copies, cut = (8 if attempt == 2 else 16), (trim if attempt else 0)
        row_bytes, slack = ((3 * S - cut) | 1) * 4, (S + 32) * 4
        bound = THREADS // copies * 16 * cpr
        if nrows * 128 * copies + nrows * row_bytes + slack > lds_bytes or bound > 65535:
            continue

        def bytes_for(nt, pc):
            rows = nrows - 1 + nt
            return rows * 128 * copies + pc * (rows * row_bytes + slack)
        ntrash = next((nt for nt in (8, 4, 2) if bytes_for(nt, 1) <= lds_bytes), 1)
        pos_copies = next((pc for pc in (4, 2) if cpr <= 12 and bytes_for(ntrash, pc) <= lds_bytes), 1)
        return done(route='v3', attempt=attempt, dn=copies, cut=cut, ntrash=ntrash, pos_copies=pos_copies,
                    dn_flush_iters=max(1, 65535 // bound), lds=bytes_for(ntrash, pos_copies))
    # kbbq_accumulate_band_dev: the first-generation kernel with the whole 43 x (2S | 1) table in the LDS, else its column tiles
    lds = ((NQ * (2 * S | 1) + 1) & ~1) * 4 + NQ * 16 * 8
    return done(route='plain' if lds <= lds_bytes else 'tiled', lds=lds)


# ---- hand-made reads ------------------------------------------------------------------------------------------------------------

def _de_bruijn5():
    """All 25 ordered pairs of 5 symbols in one cycle of 25."""
    k, n = 5, 2
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return np.array(seq, dtype=np.int64)


DB = _de_bruijn5()


def planes(lengths, second, rg, pitch, base, qual, err):
    """One-read-per-row planes from per-row lengths / second-in-pair flags / read groups and functions of (row r, position):
    base -> index into ACGTN, qual -> 0..42, err -> the corrected base differs (it is another letter of ACGT).  Bytes past a
    read are N / N / 0, as the layout contract wants them."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    r, at = np.arange(n)[:, None], np.arange(pitch)[None, :]
    inside = at < lengths[:, None]
    idx = np.broadcast_to(base(r, at), (n, pitch)) % 5
    seq = np.where(inside, LETTERS[idx], ord('N')).astype(np.uint8)
    wrong = LETTERS[np.where(idx == 4, (r + at) % 4, (idx + 1 + (r + at) % 3) % 4)]
    cseq = np.where(inside & np.broadcast_to(err(r, at), (n, pitch)), wrong, seq).astype(np.uint8)
    q = np.where(inside, 33 + np.broadcast_to(qual(r, at), (n, pitch)) % NQ, 0).astype(np.uint8)
    meta = (lengths | (np.asarray(rg, dtype=np.int64) << 16) | (np.asarray(second, dtype=np.int64) << 31)).astype(np.uint32)
    return seq, cseq, q, meta


DIRECTED_ROWS = 16 * 64 + 65            # one full workgroup iteration (16 waves x 64 rows), a full block and a block of one row
EDGE_ROW = 64 + 63                      # the second-in-pair read of length s_min that carries the errors at both of its ends


def directed_reads(S, s_min, pitch=None, rows=DIRECTED_ROWS, R=3):
    """The directed reads of one shape (tests/test_gpu_k1_routes.py says what they carry; check_directed asserts it)."""
    assert 1 <= s_min <= S and rows >= 4 * 64 and R == 3
    pitch = pitch or (S + 15) // 16 * 16
    r = np.arange(rows)
    lengths = s_min + (r * 7919 + 13) % (S - s_min + 1)
    second = (r // 2 + r // 64) & 1
    rg = 2 * ((r // 3 + r // 64) % 2)                    # groups 0 and 2 mixed inside every block; group 1 stays empty
    # the longest and the shortest read, first and second in pair, in lanes 0 and 63 of a block, the first row and the last one
    combos = [(S, 0), (s_min, 1), (S, 1), (s_min, 0)]
    edge_rows = [0, 63, 64, EDGE_ROW, 128, 191, 192, 255, rows - 1 - (rows - 1) % 64 - 1, rows - 1]
    for i, row in enumerate(edge_rows):
        lengths[row], second[row] = combos[(i + i // 2) % 4] if row != EDGE_ROW else (s_min, 1)
    lengths[[5, 70, rows - 62]] = 0                      # empty reads
    hi = 30                                              # a quality every threshold of the tests counts
    L = lengths[:, None]

    def qual(rr, at):
        q = (at * 3 + 5 * rr) % NQ
        q = np.where(at == 0, rr % NQ, q)                                         # every quality at a first base ...
        q = np.where(at == L - 1, (rr * 7 + 3) % NQ, q)                           # ... and at a last one
        return np.where((rr == EDGE_ROW) & ((at == 0) | (at == s_min - 1)), hi, q)

    def err(rr, at):
        return ((at + 3 * rr) % 7 == 0) | ((rr == EDGE_ROW) & ((at == 0) | (at == s_min - 1)))
    return planes(lengths, second, rg, pitch, base=lambda rr, at: DB[(at + 7 * rr) % 25], qual=qual, err=err)


def check_directed(p, S, s_min, R=3):
    """The asserts on the inputs of directed_reads(S, s_min): part of every test that runs them."""
    seq, cseq, qual, meta = p
    n = len(meta)
    m = meta.astype(np.int64)
    length, rg, second = m & 0xFFFF, (m >> 16) & 0x7FFF, m >> 31
    lane = np.arange(n) % 64
    for want_len in (S, s_min):
        for sec in (0, 1):
            hit = (length == want_len) & (second == sec)
            assert (hit & (lane == 0)).any() and (hit & (lane == 63)).any(), (want_len, sec)
    assert length[0] in (S, s_min) and length[n - 1] in (S, s_min) and n % 64 == 1
    full = length[length > 0]
    assert full.min() == s_min and full.max() == S and (length == 0).any()
    if s_min < S:                                        # no sorted order, either way
        d = np.diff(full)
        assert (d > 0).any() and (d < 0).any()
    assert set(np.unique(rg)) == {0, 2} and R == 3       # three read groups, the middle one empty
    for b in range((n + 63) // 64 - 1):                  # ... and both in every full block: the kernel compacts the lanes
        assert set(rg[64 * b:64 * b + 64]) == {0, 2}
    rows = np.nonzero(length)[0]
    assert set(qual[rows, 0] - 33) == set(range(NQ)) and set(qual[rows, length[rows] - 1] - 33) == set(range(NQ))
    code = _CODE[seq]
    pairs_seen = set()
    for i in rows:
        c = code[i, :length[i]]
        pairs_seen |= set(zip(c[:-1].tolist(), c[1:].tolist()))
    assert pairs_seen == {(a, b) for a in range(5) for b in range(5)}
    e = EDGE_ROW
    assert length[e] == s_min and second[e] == 1 and seq[e, 0] != cseq[e, 0] and seq[e, s_min - 1] != cseq[e, s_min - 1]
    assert qual[e, 0] - 33 == 30 and qual[e, s_min - 1] - 33 == 30
    inside = np.arange(seq.shape[1])[None, :] < length[:, None]
    assert np.all(seq[~inside] == ord('N')) and np.all(cseq[~inside] == ord('N')) and not qual[~inside].any()


def one_bin_reads(S, pitch, rows, errors):
    """`rows` first-in-pair reads of length S in read group 0, every base A at quality 30; errors: every corrected base is C."""
    return planes(np.full(rows, S), np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64), pitch,
                  base=lambda r, at: 0 * at, qual=lambda r, at: 30 + 0 * at, err=lambda r, at: (at >= 0) & bool(errors))


def pack_pairs(p, S):
    """Mate-pair rows (character planes) of one-read-per-row planes whose reads alternate as the two halves of a row, all of
    length S; the row's sidecar word is 2S + 1 | rg << 16."""
    seq, cseq, qual, meta = p
    n = len(meta)
    assert n % 2 == 0 and np.all((meta & 0xFFFF) == S) and np.all((meta[0::2] >> 16) & 0x7FFF == (meta[1::2] >> 16) & 0x7FFF)
    pitch = pair_pitch(2 * S)
    out = []
    for plane, fill in ((seq, ord('N')), (cseq, ord('N')), (qual, 0)):
        rows = np.full((n // 2, pitch), fill, dtype=np.uint8)
        rows[:, :S] = plane[0::2, :S]
        rows[:, S + 1:2 * S + 1] = plane[1::2, :S]
        out.append(rows)
    pmeta = ((2 * S + 1) | (((meta[0::2].astype(np.int64) >> 16) & 0x7FFF) << 16)).astype(np.uint32)
    return out[0], out[1], out[2], pmeta
