"""
GPU tests (-m gpu) of KBBQ_ROWS_ERRBIT in K1 and K2 (include/kbbq_hip.h; csrc/kbbq_kernels_v3.h k1v3_body `EB`,
csrc/kbbq_k2_tile.h k2t_apply_pair `EB`): on 4-bit mate-pair rows of 19 / 13 chunks bit 3 of a seq nibble says "the
corrected read differs here", K1 takes its error count from that bit and loads no corrected plane, K2 masks the bit away.

K1: the count tables equal the CPU oracle's on the same reads AND those of `accumulate` on the layout without the flag
(`lay_out(errbit=False)`: the two-plane kernels), exactly.  Every errbit batch is tallied with its corrected plane taken
away (`cseq = None`: the kernel is handed a NULL pointer).  Shapes are those of test_gpu_k1_uniform_blocks.py and
test_gpu_k1_block_pipeline.py: 2048 + e pair rows (32 full 64-row blocks and nothing / a partial block / a 33rd block), one
read group, rows grouped by read group (a slice edge inside a block, and one at 64 m + 1), twin rows, a SPLIT launch, a
batch long enough to cross a flush of the context table in one workgroup, one block made non-uniform by a short mate.
Corrections are placed (on top of the generator's own) on every nibble position of a chunk, on both neighbours of the
separator, as N -> letter and letter -> N, and one whole block is left without any.
K2: 432 rows as in test_gpu_k2_pair_forms.py, corrections on the base before a wave's first chunk (the `before` byte), on
lane 63's last base (the readlane carry) and on both neighbours of the separator; every output byte equals `apply` on the
layout without the flag and the CPU oracle, stored in grouped order and through the permutation, by the short-lived and
the persistent kernel.
"""
import numpy as np
import pytest

from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

MANY = 256           # tables of 256 read groups: ONE workgroup per slice on 256 compute units (test_gpu_k1_uniform_blocks.py)
OTHER = {ord('A'): ord('C'), ord('C'): ord('G'), ord('G'): ord('T'), ord('T'): ord('A')}


def _host(b, n):
    return [x[:n].cpu().numpy().copy() for x in (b.seq, b.cseq, b.qual)] + [b.meta[:n].cpu().numpy().view(np.uint32).copy()]


def _correct(seq, cseq, qual, read, pos, to=None):
    """Base `pos` of `read` becomes a counted correction (another letter in cseq, or `to`)."""
    if seq[read, pos] == ord('N') and to is None:
        seq[read, pos] = ord('A')
    cseq[read, pos] = OTHER[int(seq[read, pos])] if to is None else to
    qual[read, pos] = 33 + 30


def _reads(dev, S, rows, R=1, seed=0, twins=False):
    """2 * rows synthetic reads as host planes with the corrections the module's docstring lists."""
    n = 2 * rows
    b = dev.ReadBatch.synthetic(0, n, n, seed=911 + S + R + seed, len_lo=S, len_hi=S, nrg=R, qlo=2)
    seq, cseq, qual, meta = _host(b, n)
    if twins:
        meta &= np.uint32(0x7FFFFFFF)
    for t in range(16):                               # low and high nibbles of every byte position of a chunk, both mates
        _correct(seq, cseq, qual, 2 * (10 + t), 32 + t)
        _correct(seq, cseq, qual, 2 * (10 + t) + 1, 48 + t)
    for r in (80, 81, 2 * 70, 2 * 70 + 1):            # both neighbours of the separator (and of the row's ends)
        _correct(seq, cseq, qual, r, 0)
        _correct(seq, cseq, qual, r, S - 1)
    seq[100, 20] = ord('N'); _correct(seq, cseq, qual, 100, 20, to=ord('A'))          # an N corrected to a letter
    seq[101, 21] = ord('C'); _correct(seq, cseq, qual, 101, 21, to=ord('N'))          # a letter corrected to N
    cseq[2 * 128:2 * 192] = seq[2 * 128:2 * 192]                                       # block 2: rows with no correction at all
    return seq, cseq, qual, meta


def _batch(dev, planes):
    seq, cseq, qual, meta = planes
    return dev.ReadBatch.from_host(seq, qual, meta, cseq=cseq)


def _laid_pair(dev, planes, R, S, keep=False):
    """(the ERRBIT layout without its corrected plane, the two-plane layout) of the same reads."""
    eb = dev.lay_out(_batch(dev, planes), R, S, packed=True, keep_corrected=keep)
    plain = dev.lay_out(_batch(dev, planes), R, S, packed=True, errbit=False)
    assert eb.nib and eb.errbit and isinstance(eb, dev.PairBatch) and (eb.cseq is None) == (not keep)
    assert plain.nib and not plain.errbit and plain.cseq is not None and eb.layout_key() == plain.layout_key() == 'pairs_nib'
    return eb, plain


def _tally(dev, batch, R, S, minscore=6, dmin=None):
    t = dev.Tables(R, 2 * S)
    dev.accumulate(batch, t, minscore, dinuc_minscore=dmin)
    return t.to_host()


def _same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize('extra', [0, 1, 63, 64])
@pytest.mark.parametrize('S', [150, 100])
def test_full_blocks_and_what_follows_them(dev, oracle, S, extra):
    import torch
    planes = _reads(dev, S, 2048 + extra)
    eb, plain = _laid_pair(dev, planes, 1, S, keep=True)
    # the planes: bits 0-2 are the two-plane layout's codes, bit 3 is where its two planes differ, nothing else
    x = plain.seq ^ plain.cseq
    bit3 = ((x & 0x0F) != 0).to(torch.uint8) * 0x08 + ((x & 0xF0) != 0).to(torch.uint8) * 0x80
    assert torch.equal(eb.seq, plain.seq | bit3) and torch.equal(eb.cseq, plain.cseq) and int(bit3.sum()) > 0
    assert torch.equal(eb.chars('seq'), plain.chars('seq')) and torch.equal(eb.qual, plain.qual) and torch.equal(eb.meta, plain.meta)
    eb.cseq = None
    want = oracle.accumulate(*planes, 1, S, minscore=6)[5:9]
    assert int(want[0].sum()) > 100                   # errors are counted
    got = _tally(dev, eb, 1, S)
    _same(got, want)
    _same(got, _tally(dev, plain, 1, S))


@pytest.mark.parametrize('S', [150, 100])
def test_rows_grouped_by_read_group(dev, oracle, S):
    R = 2
    planes = _reads(dev, S, 2048 + 37, R=R)
    eb, plain = _laid_pair(dev, planes, R, S)
    seg = eb.seg.cpu().numpy()
    assert int(seg[1]) >= 128 and int(seg[2] - seg[1]) >= 128 and int(seg[1]) % 64       # the slice boundary inside a block
    want = oracle.accumulate(*planes, R, S, minscore=6)[5:9]
    got = _tally(dev, eb, R, S)
    _same(got, want)
    _same(got, _tally(dev, plain, R, S))


@pytest.mark.parametrize('S', [150, 100])
def test_a_slice_edge_one_row_past_a_block(dev, oracle, S):
    R, rows = 2, 2048
    seq, cseq, qual, meta = _reads(dev, S, rows)
    edge = 64 * 5 + 1                                  # group 0 owns rows [0, 64 m + 1): its last block holds ONE row
    meta[2 * edge:] |= np.uint32(1 << 16)
    planes = (seq, cseq, qual, meta)
    eb, plain = _laid_pair(dev, planes, R, S)
    assert eb.seg.cpu().numpy().tolist() == [0, edge, rows]
    want = oracle.accumulate(*planes, R, S, minscore=6)[5:9]
    got = _tally(dev, eb, R, S)
    _same(got, want)
    _same(got, _tally(dev, plain, R, S))


def test_twin_rows(dev, oracle):
    S = 150
    planes = _reads(dev, S, 2048 + 1, twins=True)
    planes = tuple(p[:-1] for p in planes)             # an odd number of single-end reads: the last row's second half is padding
    eb, plain = _laid_pair(dev, planes, 1, S)
    assert eb.twins and plain.twins and eb.n == 2049
    want = oracle.accumulate(*planes, 1, S, minscore=6)[5:9]
    got = _tally(dev, eb, 1, S)
    _same(got, want)
    _same(got, _tally(dev, plain, 1, S))


@pytest.mark.parametrize('S', [150, 100])
def test_a_split_launch(dev, oracle, S):
    """dinuc_minscore > minscore: the SPLIT instances -- cycle tables the oracle's at minscore, context tables at dinuc_minscore."""
    R = 2
    planes = _reads(dev, S, 2048 + 37, R=R, seed=1)
    eb, plain = _laid_pair(dev, planes, R, S)
    pos = oracle.accumulate(*planes, R, S, minscore=6)[5:9]
    ctx = oracle.accumulate(*planes, R, S, minscore=12)[5:9]
    got = _tally(dev, eb, R, S, 6, dmin=12)
    _same(got, (pos[0], pos[1], ctx[2], ctx[3]))
    _same(got, _tally(dev, plain, R, S, 6, dmin=12))


@pytest.mark.parametrize('short_row', [None, 64 * 16 + 63])
@pytest.mark.parametrize('S', [150, 100])
def test_one_workgroup_across_a_flush_of_the_context_table(dev, oracle, S, short_row):
    """Tables of 256 read groups on ungrouped rows: one workgroup per slice, so that wave w walks blocks w, 16 + w, ... and
    the 2048 + 1088 rows cross the flush of the 16-bit context table (every 3 / 4 iterations of 1024 rows) with the next
    block's loads in flight.  short_row: that row holds its first mate only -- its block (wave 0's second) takes the
    general loop between two uniform blocks: fed -> general -> cold start of the uniform loop."""
    R, rows = MANY, 2048 + 1088
    assert dev.context(None).compute_units // MANY <= 1
    seq, cseq, qual, meta = _reads(dev, S, rows, seed=2)
    if short_row is not None:
        qual[2 * short_row + 1, :S] = 33               # for the oracle the missing mate is a read that reaches no threshold
    planes = (seq, cseq, qual, meta)
    eb, plain = _laid_pair(dev, planes, 1, S)
    assert eb.seg is None
    if short_row is not None:
        for laid in (eb, plain):
            laid.qual[short_row, S:] = 0
            laid.meta[short_row] = S
    want = oracle.accumulate(*planes, R, S, minscore=6)[5:9]
    got = _tally(dev, eb, R, S)
    _same(got, want)
    _same(got, _tally(dev, plain, R, S))


@pytest.mark.parametrize('row', [64 * 17 + 9, 2048 + 20])      # in a uniform block / in the partial block (the general loop)
@pytest.mark.parametrize('nibble', [0x50, 0x60, 0x70, 0xD0, 0xE0, 0xF0])
def test_a_nibble_that_is_no_code_is_reported_with_and_without_bit_3(dev, row, nibble):
    S = 150
    planes = _reads(dev, S, 2048 + 37, seed=3)
    eb, _ = _laid_pair(dev, planes, 1, S)
    eb.seq[row, 19] = (int(eb.seq[row, 19]) & 0x0F) | nibble
    with pytest.raises(dev.N.LutNeedsCheckedApply):
        dev.accumulate(eb, dev.Tables(1, 2 * S))


# ---------------------------------------------------------------------------------------------------------------- K2
K2_ROWS = 432


def _k2_reads(oracle, S, R):
    n = 2 * K2_ROWS
    seq, _, qual, meta = oracle.synth(0, n, n, 2000 + S + R, S, S, 1, 0, 41)
    seq, qual, meta = seq.copy(), qual.copy(), meta.copy()
    if R > 1:
        rg = (np.arange(K2_ROWS) * 5 % 7 % R).astype(np.uint32)
        meta = (meta & np.uint32(0x8000FFFF)) | (np.repeat(rg, 2) << np.uint32(16))
    seq[seq == ord('N')] = ord('A')
    cseq = seq.copy()
    ppitch = (2 * S + 1 + 15) // 16 * 16

    def flip(byte):                                    # byte offset in the (ungrouped) pair-row plane -> a corrected base
        row, p = divmod(byte, ppitch)
        if p < S:
            cseq[2 * row, p] = OTHER[int(seq[2 * row, p])]
        elif S < p <= 2 * S:
            cseq[2 * row + 1, p - S - 1] = OTHER[int(seq[2 * row + 1, p - S - 1])]
    for c in range(64, K2_ROWS * (ppitch // 16), 64):
        flip(16 * c - 1)                               # lane 63's last base; every 4th of them is the base before a wave's first chunk
        flip(16 * c)
    for r in range(0, n, 2):                           # both neighbours of every separator
        cseq[r, S - 1] = OTHER[int(seq[r, S - 1])]
        cseq[r + 1, 0] = OTHER[int(seq[r + 1, 0])]
    return seq, cseq, qual, meta


@pytest.mark.parametrize('R,restore', [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize('S', [150, 100])
def test_k2_ignores_the_error_bit(dev, oracle, monkeypatch, S, R, restore):
    import torch
    seq, cseq, qual, meta = _k2_reads(oracle, S, R)
    tabs = oracle.accumulate(seq, cseq, qual, meta, R, S, minscore=6)
    model = (tabs[0],) + tuple(oracle.get_delta_qs(*tabs))
    lut, shape = dev.build_lut(*model)
    assert shape[3] == dev.N.APPLY_FAST
    lut = dev.lut_to_device(lut)
    want = oracle.apply(seq, qual, meta, *model)[:, :S] + 33
    eb, plain = _laid_pair(dev, (seq, cseq, qual, meta), R, S)
    assert eb.n == K2_ROWS and int((eb.seq & 0x88).ne(0).sum()) >= 2 * K2_ROWS
    if R == 1:                                         # rows in input order: the bits sit where the docstring says
        last = (eb.seq.reshape(-1, 8)[:, 7] & 0x80).ne(0).cpu().numpy()          # bit 3 of every chunk's last base
        p = 16 * (np.arange(last.size) % (eb.pitch // 16)) + 15                   # that base's offset in its row
        is_base = (p < S) | ((p > S) & (p <= 2 * S))                              # (no separator, no padding)
        for every in (64, 256):                                                   # lane 63's last base / the base before a wave's first chunk
            assert last[every - 1::every][is_base[every - 1::every]].all() and is_base[every - 1::every].sum() >= 0.8 * (last.size // every)
    got = dev.apply(eb, lut, shape, restore_order=restore)
    assert torch.equal(got, dev.apply(plain, lut, shape, restore_order=restore))
    rows = got if (restore or R == 1) else dev.ungroup(eb, got)
    out = eb.unpack(rows, 160 if S == 150 else 112)[:2 * K2_ROWS].cpu().numpy()
    assert np.array_equal(out[:, :S], want) and not out[:, S:].any()
    # ... and the persistent kernel on the same planes
    monkeypatch.setenv('KBBQ_K2_TILE', '0')
    assert torch.equal(dev.apply(eb, lut, shape, restore_order=restore), got)
