"""
GPU tests (-m gpu) of K1's software pipeline across uniform blocks on 4-bit mate-pair rows (csrc/kbbq_kernels_v3.h,
k1v3_body, the `KJ > 0` instances: 19 and 13 chunks per row).  While a wave bins the last step of a uniform 64-row block it
already has the sidecar words and the step-0 loads of ITS next block in flight -- across a flush of the context table too
-- and the ballot on those sidecar words decides whether the step is used or dropped for the general loop; the flush of
the context table gives one bin to each thread.  A wave's next block is fetched ahead only when its 64 rows lie wholly
inside the slice.

Every case passes tables of as many read groups as the device has compute units: the launch then gives a read-group slice
ONE workgroup (launch_k1: max(1, compute units / R)), in which wave w walks blocks w, 16 + w, 32 + w, ... of the slice
one after the other -- the order the cases below are written for.  All of them run S = 150 and S = 100 (19 / 13 chunks) at
minscore 6 and are compared with the CPU oracle on the same reads, exactly.
"""
import numpy as np
import pytest

from test_gpu_parity import dev                      # noqa: F401  (fixture)
from test_gpu_k1_joint_rows import _planes, _same

pytestmark = pytest.mark.gpu

WAVES = 16                                            # waves of a K1 workgroup: a wave's blocks are 16 apart


def _cus(dev):
    return dev.context(None).compute_units


def _host(b, n):
    return [x[:n].cpu().numpy() for x in (b.seq, b.cseq, b.qual)] + [b.meta[:n].cpu().numpy().view(np.uint32)]


def _one_workgroup_per_slice(dev, R):
    assert max(1, _cus(dev) // R) == 1


# ---- 1. block sequences of a wave ------------------------------------------------------------------------------------------
# 2048 + e rows: 32 full blocks -- two iterations of the workgroup -- and e more rows: nothing, a partial block (1 or 63
# rows: wave 0's third block takes the general loop and is NOT fetched ahead) or a 33rd full block (wave 0 alone makes a
# third iteration).  The rows named by `where` are made non-uniform, one to a block:
#   none        every wave: uniform -> uniform (the step fetched ahead is used)
#   block0      wave 0: general -> uniform (nothing was fetched ahead for block 16) [-> block 32]
#   block16     wave 0: uniform -> general (the step fetched ahead is dropped) [-> uniform or partial]
#   iteration1  every wave: uniform -> general: sixteen steps dropped, one row in each of blocks 16 .. 31
#   last_full   the last full block (31, or 32 when e = 64): a dropped step at the end of the rows
EXTRA = [0, 1, 63, 64]


def _odd_rows(where, rows):
    last_full = rows // 64 - 1
    return {'none': [],
            'block0': [5],
            'block16': [64 * 16 + 63],
            'iteration1': [64 * (16 + w) + (7 * w + 3) % 64 for w in range(WAVES)],
            'last_full': [64 * last_full + 31]}[where]


@pytest.fixture(scope='module')
def sequence_reads(dev):
    """The reads of the block-sequence cases: the longest shape, made once per S; a case takes the first 2048 + e pairs."""
    return {S: dev.ReadBatch.synthetic(0, 2 * (2048 + 64), 2 * (2048 + 64), seed=1009 + S, len_lo=S, len_hi=S, nrg=1, qlo=2)
            for S in (150, 100)}


def _first_pairs(dev, b, pairs):
    seq, cseq, qual, meta = _host(b, 2 * pairs)
    return dev.ReadBatch.from_host(seq, qual, meta, cseq=cseq)


@pytest.mark.parametrize('how', ['short_mate', 'other_group'])
@pytest.mark.parametrize('where', ['none', 'block0', 'block16', 'iteration1', 'last_full'])
@pytest.mark.parametrize('extra', EXTRA)
@pytest.mark.parametrize('S', [150, 100])
def test_block_sequences_of_a_wave(dev, oracle, sequence_reads, S, extra, where, how):
    if where == 'none' and how == 'other_group':
        how = 'short_mate'                                      # no odd row either way: the same run
    R, rows = _cus(dev), 2048 + extra
    _one_workgroup_per_slice(dev, R)
    odd = _odd_rows(where, rows)
    assert all(r < (rows // 64) * 64 for r in odd) and len({r // 64 for r in odd}) == len(odd)
    b = _first_pairs(dev, sequence_reads[S], rows)
    for row in odd:
        if how == 'short_mate':
            b.qual[2 * row + 1, :S] = 33                        # for the oracle: a mate none of whose bases is counted
        else:
            b.meta[2 * row:2 * row + 2] |= 1 << 16              # a pair of read group 1 among those of read group 0
    want = oracle.accumulate(*_host(b, b.n), R, S, minscore=6)[5:9]
    laid = dev.lay_out(b, 1, S, packed=True)                    # R = 1: the rows stay in input order, no `seg`
    assert laid.nib and isinstance(laid, dev.PairBatch) and laid.seg is None and laid.n == rows
    if how == 'short_mate':
        for row in odd:                                         # the row holds its first mate only
            laid.qual[row, S:] = 0
            laid.meta[row] = S
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t, 6)
    got = t.to_host()
    _same(got, want)
    assert (int(got[1][1].sum()) > 0) == (how == 'other_group' and len(odd) > 0)           # slice 1 found its rows, nothing else
    assert int(got[1][2:].sum()) == 0


# ---- 2. slice edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [150, 100])
def test_blocks_behind_a_slice_belong_to_the_next_one(dev, oracle, S):
    """Rows grouped by read group, three groups with boundaries at 64 * 33 + 1 and 64 * 65 + 63: behind the last full block of
    group 0 (its block 32) one row of its own is left, behind that of group 1 (its block 31) 62 of them -- the rest of either
    64-row block holds the NEXT group's rows, and so do the blocks 16 further on that the waves of the last iteration
    would fetch ahead.  None of that may be counted for the group: the tables are exact per group."""
    R = _cus(dev)
    _one_workgroup_per_slice(dev, R)
    n0, n1, n2 = 64 * 33 + 1, 64 * 32 + 62, 64 * 17 + 5
    pairs = n0 + n1 + n2
    b = dev.ReadBatch.synthetic(0, 2 * pairs, 2 * pairs, seed=2003 + S, len_lo=S, len_hi=S, nrg=1, qlo=2)
    group = np.repeat([0, 1, 2], [n0, n1, n2])
    rng = np.random.default_rng(5)
    rng.shuffle(group)                                          # the layout pass gathers the groups' rows
    import torch
    bits = torch.from_numpy(np.repeat(group << 16, 2)).to(device=b.meta.device, dtype=b.meta.dtype)
    b.meta[:2 * pairs] |= bits
    want = oracle.accumulate(*_host(b, b.n), R, S, minscore=6)[5:9]
    laid = dev.lay_out(b, R, S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch) and laid.seg is not None
    seg = laid.seg.cpu().numpy()
    assert seg[:4].tolist() == [0, n0, n0 + n1, pairs] and (seg[3:] == pairs).all()
    assert seg[1] % 64 == 1 and seg[2] % 64 == 63
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t, 6)
    got = t.to_host()
    _same(got, want)
    for g, n in enumerate((n0, n1, n2)):                        # (what _same has checked, said per group)
        assert 0 < int(got[1][g].sum()) == int(want[1][g].sum()) <= 2 * S * n
    assert int(got[1][3:].sum()) == 0


# ---- 3. across a flush of the context table, a step fetched ahead in flight ----------------------------------------------------

def _flush_rows(S, extra):
    KJ = (2 * S + 1 + 15) // 16
    threads, copies = 1024, 16
    flush_iters = max(1, 65535 // ((threads // copies) * 16 * KJ))      # accumulate_rows: K1v3Params::dn_flush_iters
    assert flush_iters == {19: 3, 13: 4}[KJ]
    assert (flush_iters + 1) * (threads // copies) * 16 * KJ > 65535     # one more iteration without a flush could overflow a half
    return (threads // 64) * 64 * flush_iters + extra


def _flush_planes(S, extra, errors):
    """The shape of test_gpu_k1_joint_rows.py::test_one_workgroup_past_a_context_flush: every base A at quality 30, so that
    all counts of a copy land in ONE 16-bit half, which is full to the last iteration before the flush; `extra` rows behind
    it -- one row (a partial block), a uniform block, a whole iteration and a block: their step 0 was fetched ahead of the
    flush where they are full blocks."""
    rows = _flush_rows(S, extra)
    err = (lambda r, at: at % 7 == 0) if errors else (lambda r, at: at < 0)
    return rows, _planes(S, rows, base=lambda r, at: 0 * at, qual=lambda r, at: 30 + 0 * at, err=err)


def _run_flush(dev, planes, S, R, dmin=None):
    b = dev.ReadBatch.from_host(planes[0], planes[2], planes[3], cseq=planes[1])
    laid = dev.lay_out(b, 1, S, packed=True)
    assert laid.nib and isinstance(laid, dev.PairBatch) and not laid.twins and laid.seg is None
    t = dev.Tables(R, 2 * S)
    dev.accumulate(laid, t, 6, dinuc_minscore=dmin)
    return t.to_host()


def _check_flush(got, want, S, rows, errors):
    _same(got, want)
    nerr = sum(1 for mate in (0, 1) for i in range(S) if (i + (S + 1) * mate) % 7 == 0) if errors else 0
    nerr_ctx = sum(1 for mate in (0, 1) for i in range(1, S) if (i + (S + 1) * mate) % 7 == 0) if errors else 0
    assert got[1].sum() == 2 * S * rows and got[3].sum() == 2 * (S - 1) * rows       # totals: no half carried away ...
    assert got[0].sum() == nerr * rows and got[2].sum() == nerr_ctx * rows           # ... or into the errors
    assert got[3][0, 30, 0] == 2 * (S - 1) * rows and got[2][0, 30, 0] == nerr_ctx * rows      # all of them AA at quality 30, read group 0


@pytest.mark.parametrize('errors', [False, True])
@pytest.mark.parametrize('extra', [1, 64, 1088])
@pytest.mark.parametrize('S', [150, 100])
def test_across_a_context_flush_with_a_step_in_flight(dev, oracle, S, extra, errors):
    R = _cus(dev)
    _one_workgroup_per_slice(dev, R)
    rows, planes = _flush_planes(S, extra, errors)
    want = oracle.accumulate(*planes, R, S, minscore=6)[5:9]
    _check_flush(_run_flush(dev, planes, S, R), want, S, rows, errors)


@pytest.mark.parametrize('S', [150, 100])
def test_across_a_context_flush_split(dev, oracle, S):
    """The SPLIT instance (dinuc_minscore 20 above minscore 6) on the same shape: quality 30 passes both thresholds."""
    R = _cus(dev)
    rows, planes = _flush_planes(S, 64, True)
    pos = oracle.accumulate(*planes, R, S, minscore=6)[5:9]
    ctx = oracle.accumulate(*planes, R, S, minscore=20)[5:9]
    _check_flush(_run_flush(dev, planes, S, R, dmin=20), (pos[0], pos[1], ctx[2], ctx[3]), S, rows, True)
