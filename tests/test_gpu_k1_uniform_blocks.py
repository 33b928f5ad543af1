"""
GPU tests (-m gpu) of K1's uniform-block loop on 4-bit mate-pair rows (csrc/kbbq_kernels_v3.h, k1v3_body, the
`NIB && KJ > 0` instances: 19 and 13 chunks per row, with and without SPLIT).  A 64-row block whose rows are all complete
pairs of the common length in the slice's read group takes that loop; every other block takes the general one.  The
kernel keeps no switch between the two, so every case is compared with the CPU oracle on the same reads, exactly.

Shapes: 64 * 16 * 2 + 64 + 37 pair rows -- 33 full blocks and a partial one (the general loop).  The launch makes no more
workgroups than there are iterations, so with 1 or 2 read groups every wave walks ONE block; the mixed-block cases below
run with one workgroup per slice, where a wave walks three.  With 2 read groups (rows grouped by `seg`) a slice boundary
falls inside a 64-row block.
"""
import numpy as np
import pytest

from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PAIRS = 64 * 16 * 2 + 64 + 37
LAST_FULL = (PAIRS // 64 - 1) * 64                   # first row of the last full block: the one before the partial block
# The mixed-block cases run on UNGROUPED rows against tables of 256 read groups: the launch gives a read-group slice
# max(1, compute units / 256) workgroups -- ONE on the 256 compute units of an MI355X -- so that wave w of slice 0 walks
# blocks w, 16 + w and 32 + w (the partial block 33 for w = 1) one after the other.  ONE row per run is made non-uniform,
# so that exactly one block of one wave takes the general loop between (before, after) uniform blocks of that wave:
MANY = 256
ODD_ROW = {
    'start': 5,                          # block 0:  wave 0 goes general, fast, fast
    'middle': 64 * 16 + 63,              # block 16: wave 0 goes fast, general, fast
    'middle_then_partial': 64 * 17 + 20,     # block 17: wave 1 goes fast, general, general (the partial block)
    'before_partial': LAST_FULL + 31,    # block 32: wave 0 goes fast, fast, general
}


def _host(b, n):
    return [x[:n].cpu().numpy() for x in (b.seq, b.cseq, b.qual)] + [b.meta[:n].cpu().numpy().view(np.uint32)]


def _reads(dev, S, R, seed=0):
    n = 2 * PAIRS
    return dev.ReadBatch.synthetic(0, n, n, seed=311 + S + R + seed, len_lo=S, len_hi=S, nrg=R, qlo=2)


def _same(tables, want):
    for got, w in zip(tables.to_host(), want):
        assert np.array_equal(got, w)


@pytest.fixture(scope='module')
def cases(dev, oracle):
    """The reads of every (S, R) and the oracle's tables for them, computed once (read-only)."""
    out = {}
    for S in (150, 100):
        for R in (1, 2):
            b = _reads(dev, S, R)
            host = _host(b, b.n)
            out[S, R] = (b, host, {6: oracle.accumulate(*host, R, S, minscore=6)[5:9]})
    return out


def _want(oracle, case, S, R, minscore):
    _, host, wants = case
    if minscore not in wants:
        wants[minscore] = oracle.accumulate(*host, R, S, minscore=minscore)[5:9]
    return wants[minscore]


@pytest.mark.parametrize('R', [1, 2])
@pytest.mark.parametrize('S', [150, 100])
def test_full_blocks_a_partial_block_and_a_slice_boundary(dev, oracle, cases, S, R):
    b, _, wants = cases[S, R]
    laid = dev.lay_out(b, R, S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch) and laid.n == PAIRS and (laid.seg is not None) == (R > 1)
    if R > 1:
        seg = laid.seg.cpu().numpy()
        assert int(seg[1]) >= 128 and PAIRS - int(seg[1]) >= 128 and int(seg[1]) % 64       # full blocks in both slices, the boundary inside one
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t)
    _same(t, wants[6])


@pytest.mark.parametrize('S', [150, 100])
@pytest.mark.parametrize('minscore,dmin', [(6, 12), (6, 20), (12, 6)])
def test_split_thresholds(dev, oracle, cases, S, minscore, dmin):
    """dinuc_minscore != minscore: a base is counted from `minscore` up, and its context only from the larger of the two
    thresholds up -- the cycle tables are the oracle's at minscore, the context tables the oracle's at max(minscore,
    dmin).  The launch picks a SPLIT instance when dinuc_minscore > minscore: (6, 12) and (6, 20) run one, (12, 6) is the
    other side of that choice -- the plain instance, whose context threshold is the counting one."""
    R = 2
    b = cases[S, R][0]
    pos = _want(oracle, cases[S, R], S, R, minscore)
    ctx = _want(oracle, cases[S, R], S, R, max(minscore, dmin))
    laid = dev.lay_out(b, R, S, packed=True)
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t, minscore, dinuc_minscore=dmin)
    _same(t, (pos[0], pos[1], ctx[2], ctx[3]))


@pytest.mark.parametrize('where', list(ODD_ROW))
@pytest.mark.parametrize('S', [150, 100])
def test_a_row_without_its_second_mate_among_full_blocks(dev, oracle, S, where):
    """One row holds its first mate only (sidecar length S, nothing behind it): its block takes the general loop, the
    other blocks of the same wave the uniform one, in the order ODD_ROW names.  For the oracle the missing mate is a read
    none of whose bases reaches any threshold."""
    R, row = MANY, ODD_ROW[where]
    b = _reads(dev, S, 1, seed=1)
    b.qual[2 * row + 1, :S] = 33
    seq, cseq, qual, meta = _host(b, b.n)
    want = oracle.accumulate(seq, cseq, qual, meta, R, S, minscore=6)[5:9]
    laid = dev.lay_out(b, 1, S, packed=True)                    # R = 1: the rows stay in input order, no `seg`
    assert laid.nib and isinstance(laid, dev.PairBatch) and laid.seg is None
    assert dev.context(laid.seq.device.index).compute_units // MANY <= 1       # one workgroup per slice: the order above holds
    laid.qual[row, S:] = 0
    laid.meta[row] = S
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t)
    _same(t, want)


@pytest.mark.parametrize('where', list(ODD_ROW))
@pytest.mark.parametrize('S', [150, 100])
def test_a_row_of_another_read_group_in_ungrouped_rows(dev, oracle, S, where):
    """Ungrouped rows (no `seg`: every slice scans all rows) with one pair of read group 1: in slice 0 its block is
    compacted to 63 rows and takes the general loop, the other blocks of the same wave the uniform one, in the order
    ODD_ROW names; slice 1 finds that one row and nothing else."""
    R, row = MANY, ODD_ROW[where]
    b = _reads(dev, S, 1, seed=2)
    b.meta[2 * row:2 * row + 2] |= 1 << 16
    seq, cseq, qual, meta = _host(b, b.n)
    want = oracle.accumulate(seq, cseq, qual, meta, R, S, minscore=6)[5:9]
    laid = dev.lay_out(b, 1, S, packed=True)                    # R = 1: the rows stay in input order
    assert laid.nib and isinstance(laid, dev.PairBatch) and laid.seg is None
    assert dev.context(laid.seq.device.index).compute_units // MANY <= 1
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t)
    _same(t, want)
    assert int(t.to_host()[1][1].sum()) > 0                     # slice 1 counted its row


def test_an_odd_single_end_read_in_a_full_block(dev, oracle):
    """Single-end reads two to a row, an odd number of them, the rows a multiple of 64: the last row's second half is
    padding inside a block that is uniform by its sidecar -- the padding counts nothing on either loop."""
    S, R = 150, 1
    n = 2 * 64 * 17 - 1
    b = dev.ReadBatch.synthetic(0, n, n, seed=77, len_lo=S, len_hi=S, nrg=R)
    b.meta.bitwise_and_(0x7FFFFFFF)
    seq, cseq, qual, meta = _host(b, n)
    want = oracle.accumulate(seq, cseq, qual, meta, R, S, minscore=6)[5:9]
    laid = dev.lay_out(b, R, S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch) and laid.twins and laid.n == 64 * 17
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t)
    _same(t, want)


@pytest.mark.parametrize('row', [64 * 17 + 9, PAIRS - 3])     # in a uniform block / in the partial block (the general loop): one behaviour
@pytest.mark.parametrize('S', [150, 100])
def test_a_quality_above_K_inside_a_block(dev, oracle, S, row):
    """One quality byte above 'K' (recalibrate.py:114-115): IndexError with the row's index; the 16-byte chunk that holds the
    byte counts nothing, everything else is counted -- for the oracle, the same reads with that chunk's qualities at 0."""
    R = 1
    b = _reads(dev, S, R, seed=3)
    laid = dev.lay_out(b, R, S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch)
    laid.qual[row, 35] = ord('K') + 1                          # chunk 2 of the row: positions 32 .. 47 of the first mate
    b.qual[2 * row, 32:48] = 33
    seq, cseq, qual, meta = _host(b, b.n)
    want = oracle.accumulate(seq, cseq, qual, meta, R, S, minscore=6)[5:9]
    t = dev.Tables(R, 2 * S)
    with pytest.raises(IndexError) as e:
        dev.accumulate(laid, t)
    assert e.value.read_index == row
    _same(t, want)


@pytest.mark.parametrize('row', [64 * 17 + 9, PAIRS - 3])
def test_a_corrupt_nibble_inside_a_block(dev, row):
    S = 150
    b = _reads(dev, S, 1, seed=4)
    laid = dev.lay_out(b, 1, S, packed=True)
    assert laid.nib
    laid.seq[row, 19] = (int(laid.seq[row, 19]) & 0x0F) | 0x60  # one nibble that is no code (6)
    with pytest.raises(dev.N.LutNeedsCheckedApply):
        dev.accumulate(laid, dev.Tables(1, 2 * S))
