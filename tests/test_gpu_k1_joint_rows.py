"""
GPU tests (-m gpu) of K1's joint table rows on 4-bit mate-pair rows (csrc/kbbq_kernels_v3.h, k1v3_body, the `KJ > 0`
instances: 19 and 13 chunks per row, with and without SPLIT).  One quality's cycle words and its context words share an
LDS row there, and the uniform-block loop reaches the context word from the cycle word's address by a 16-bit delta, with
an increment whose error half comes from a sub-dword min while its low half is kept.  Every case is compared with the CPU
oracle on the same reads, exactly; tests/test_gpu_k1_uniform_blocks.py covers block shapes, bad qualities and corrupt
nibbles.

Reads are made on the host, so that a case states which rows / slots / copies / byte positions it reaches: the asserts on
the inputs (before anything runs on the device) are part of the test.
"""
import numpy as np
import pytest

from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b'ACGTN', dtype=np.uint8)
CODE = {c: i for i, c in enumerate(b'ATGCN')}         # the kernel's codes (A0 T1 G2 C3, N 4): slot = 5 * code(prev) + code(cur)
ROWS = 3 * 64 + 5                                     # three uniform blocks and a partial one (the general loop), one workgroup


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


def _planes(S, rows, base, qual, err):
    """One-read-per-row character planes of `rows` pairs from functions of (pair row r, byte offset `at` in the mate-pair
    row): base(r, at) -> index into ACGTN, qual(r, at) -> quality 0..42, err(r, at) -> the corrected base differs."""
    pitch = (S + 15) // 16 * 16
    n = 2 * rows
    seq = np.full((n, pitch), ord('N'), dtype=np.uint8)
    cseq = seq.copy()
    qualp = np.zeros((n, pitch), dtype=np.uint8)
    r = np.arange(rows)[:, None]
    for mate in (0, 1):
        at = np.arange(S)[None, :] + (S + 1) * mate
        idx = np.broadcast_to(base(r, at), (rows, S)) % 5
        seq[mate::2, :S] = LETTERS[idx]
        cseq[mate::2, :S] = LETTERS[np.where(np.broadcast_to(err(r, at), (rows, S)), (idx + 1) % 4, idx)]      # another letter of ACGT
        qualp[mate::2, :S] = 33 + np.broadcast_to(qual(r, at), (rows, S))
    meta = np.full(n, S, dtype=np.uint32)
    meta[1::2] |= np.uint32(1 << 31)
    return seq, cseq, qualp, meta


def _slots_by_copy(seq, S, rows, chunks=None):
    """(slot, lane & 15) of every base of the first `rows` pair rows (full blocks: lane = chunk index in the block mod 64),
    optionally of the given chunks of a row only."""
    KJ = (2 * S + 1 + 15) // 16
    lut = np.zeros(256, dtype=np.int64)
    for c, v in CODE.items():
        lut[c] = v
    code = lut[seq[:2 * rows, :S]]
    prev = np.concatenate([np.full((2 * rows, 1), 4), code[:, :-1]], axis=1)
    slot = 5 * prev + code
    got = set()
    for mate in (0, 1):
        at = np.arange(S) + (S + 1) * mate
        j = at // 16
        for r in range(rows):
            lane15 = ((r % 64) * KJ + j) & 15
            keep = np.ones(S, bool) if chunks is None else np.isin(j, chunks)
            got |= set(zip(slot[2 * r + mate][keep].tolist(), lane15[keep].tolist()))
    return got


def _run(dev, planes, S, R, minscore, dmin=None):
    b = dev.ReadBatch.from_host(planes[0], planes[2], planes[3], cseq=planes[1])
    laid = dev.lay_out(b, 1, S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch) and not laid.twins and laid.seg is None
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t, minscore, dinuc_minscore=dmin)
    return t.to_host()


def _same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- 1. every row, slot and copy -------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def everything(oracle):
    out = {}
    for S in (150, 100):
        planes = _planes(S, ROWS,
                         base=lambda r, at: DB[(at + 7 * r) % 25],
                         qual=lambda r, at: (at + 5 * r) % 43,
                         err=lambda r, at: (at + 3 * r) % 7 == 0)
        assert _slots_by_copy(planes[0], S, 3 * 64) == {(s, c) for s in range(25) for c in range(16)}
        assert set(np.unique(planes[2][:, :S])) == set(range(33, 76))
        out[S] = (planes, {})
    return out


def _want(oracle, case, S, minscore):
    planes, wants = case
    if minscore not in wants:
        wants[minscore] = oracle.accumulate(*planes, 1, S, minscore=minscore)[5:9]
    return wants[minscore]


@pytest.mark.parametrize('minscore', [0, 6, 12])      # 44, 38 and 32 table rows
@pytest.mark.parametrize('S', [150, 100])
def test_every_row_slot_and_copy(dev, oracle, everything, S, minscore):
    """Every quality 0..42 at every chunk position, every context slot 0..24 under every copy (lane & 15), errors spread over
    all of them: the counts are the oracle's, i.e. nothing below minscore (the trash row) or with an N in its context (the
    trash slots) is counted anywhere."""
    want = _want(oracle, everything[S], S, minscore)
    assert want[1].sum() > 0 and want[0].sum() > 0 and want[3].sum() > 0 and want[2].sum() > 0
    if minscore:
        assert want[1][:, :minscore].sum() == 0
    _same(_run(dev, everything[S][0], S, 1, minscore), want)


@pytest.mark.parametrize('S', [150, 100])
def test_every_row_slot_and_copy_split(dev, oracle, everything, S):
    """The SPLIT instance (dinuc_minscore 20 above minscore 6): cycle tables as at 6, context tables as at 20."""
    pos, ctx = _want(oracle, everything[S], S, 6), _want(oracle, everything[S], S, 20)
    assert ctx[3].sum() < pos[3].sum()
    _same(_run(dev, everything[S][0], S, 1, 6, dmin=20), (pos[0], pos[1], ctx[2], ctx[3]))


# ---- 2. one error at each of the 16 byte positions of a chunk ----------------------------------------------------------------

@pytest.mark.parametrize('which', ['first', 'middle', 'last'])
@pytest.mark.parametrize('S', [150, 100])
def test_one_error_at_each_byte_of_a_chunk(dev, oracle, S, which):
    """Row r carries ONE error, at byte r % 16 of the chosen chunk (no error where that byte is the separator or padding):
    the first chunk is mate 1, the middle one holds the end of mate 1, the separator and the start of mate 2, the last one
    the end of mate 2.  The error half of the increment is written beside a low half that must stay 1 -- byte 3 of a word
    is the byte next to nothing."""
    KJ = (2 * S + 1 + 15) // 16
    j = {'first': 0, 'middle': S // 16, 'last': KJ - 1}[which]
    rows = 64 + 16 + 5                                   # a uniform block and a partial one: each byte position in both loops
    planes = _planes(S, rows,
                     base=lambda r, at: DB[(at + 7 * r) % 25] % 4,
                     qual=lambda r, at: 20 + (at + r) % 20,
                     err=lambda r, at: at == 16 * j + r % 16)
    seq, cseq = planes[0], planes[1]
    nerr = int((seq != cseq).sum())
    hit = sorted({16 * j + b for b in range(16)} - {S} - set(range(2 * S + 1, 16 * KJ)))
    assert nerr == sum(1 for r in range(rows) if 16 * j + r % 16 in hit) and len(hit) >= 9
    assert (which == 'first') == (hit[-1] < S) and (which == 'last') == (hit[0] > S)
    want = oracle.accumulate(*planes, 1, S, minscore=6)[5:9]
    assert want[0].sum() == nerr and 0 < want[2].sum() <= nerr
    got = _run(dev, planes, S, 1, 6)
    _same(got, want)
    cols = sorted(at if at < S else 2 * S - 1 - (at - S - 1) for at in hit)      # second in pair: column 2 * len - 1 - position
    assert sorted(np.nonzero(got[0].sum(axis=(0, 1)))[0].tolist()) == cols


# ---- 3. edges of the 16-bit delta ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [150, 100])
def test_rows_mostly_of_N(dev, oracle, S):
    """Rows made mostly of N: the trash slots 4, 9, 14, 19 (an N after a letter) and 20 .. 24 (anything after an N) in the first
    chunk of a row (j = 0: the largest delta) and in the last (j = KJ - 1: the smallest), under every copy; the few valid
    bins are the oracle's."""
    KJ = (2 * S + 1 + 15) // 16
    planes = _planes(S, ROWS,
                     base=lambda r, at: np.where(((at + r // 16) % 3 == 0) | (at % 11 == r % 11), (at // 3 + r // 16 + r // 4) % 4, 4),
                     qual=lambda r, at: 30 + (at + r) % 13,
                     err=lambda r, at: (at + r) % 9 == 0)
    trash = {4, 9, 14, 19, 20, 21, 22, 23, 24}
    for j in (0, KJ - 1):
        got = _slots_by_copy(planes[0], S, 3 * 64, chunks=[j])
        assert {(s, c) for s in trash for c in range(16)} <= got
    want = oracle.accumulate(*planes, 1, S, minscore=6)[5:9]
    assert 0 < want[3].sum() < want[1].sum() // 8
    _same(_run(dev, planes, S, 1, 6), want)


# ---- 4. one workgroup past a flush of the context table ---------------------------------------------------------------------

@pytest.mark.parametrize('extra', [1, 64])             # the block after the flush: one row (the general loop) / a uniform block
@pytest.mark.parametrize('S', [150, 100])
def test_one_workgroup_past_a_context_flush(dev, oracle, S, extra):
    """Every base A at one quality, no errors: all counts of a copy land in ONE 16-bit half, which the workgroup flushes every
    dn_flush_iters iterations.  Tables of as many read groups as the device has compute units give read group 0 one workgroup
    (launch_k1: max(1, compute units / R) of them), which walks 16 blocks of 64 rows per iteration: 1024 * dn_flush_iters rows
    are the last ones before a flush, `extra` more rows make the workgroup go on after it."""
    KJ = (2 * S + 1 + 15) // 16
    R = dev.context(None).compute_units
    threads, copies = 1024, 16
    flush_iters = max(1, 65535 // ((threads // copies) * 16 * KJ))      # accumulate_rows: K1v3Params::dn_flush_iters
    assert (flush_iters + 1) * (threads // copies) * 16 * KJ > 65535     # one more iteration without a flush could overflow a half
    rows = (threads // 64) * 64 * flush_iters + extra
    planes = _planes(S, rows, base=lambda r, at: 0 * at, qual=lambda r, at: 30 + 0 * at, err=lambda r, at: at < 0)
    want = oracle.accumulate(*planes, R, S, minscore=6)[5:9]
    got = _run(dev, planes, S, R, 6)
    _same(got, want)
    assert got[0].sum() == 0 and got[2].sum() == 0                      # no half carried into the errors
    assert got[1].sum() == 2 * S * rows and got[3].sum() == 2 * (S - 1) * rows
    assert got[3][0, 30, 0] == 2 * (S - 1) * rows                       # ... all of them AA at quality 30, read group 0
