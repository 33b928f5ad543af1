"""bz_deflate / bz_scan_sizes / bz_pack (csrc/kbbq_bgzf.h) on the paths that ordinary text does not enter, with inputs designed
on the CPU against a host model of the kernel (tests/bgzf_cases.py, tests/bgzf_model.py; test_bgzf_model_host.py shows that the
checks used here refuse four wrong encoders).  Every case asks three things of what the GPU wrote: zlib inflates each block to its
piece (bgzf_model.verify), the bytes are the model's -- the header comment's "a function of (text, block_bytes) alone" -- and the
path the case is about was taken, as read from the GPU's own tokens and code lengths (bgzf_model.tokens)."""
import ctypes

import numpy as np
import pytest

import bgzf_cases as C
import bgzf_model as B

pytestmark = pytest.mark.gpu


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch(text, block_bytes, offset=0):
    """(packed bytes, sizes) of `text` through kbbq_bgzf_deflate_dev, the text `offset` bytes behind a 16-byte boundary.  Nothing
    is written past the packed length or, in a slot, past the block's last word; packed is the slots' blocks joined."""
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    lib, ctx = N.load(), dev.context()
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    n = text.size
    nb = (n + block_bytes - 1) // block_bytes
    bound = int(lib.kbbq_bgzf_bound(n, block_bytes))
    room = torch.zeros(n + 32, dtype=torch.uint8, device='cuda')
    assert room.data_ptr() % 16 == 0
    d_text = room[offset:offset + n]
    d_text.copy_(torch.from_numpy(text.copy()))
    assert d_text.data_ptr() % 16 == offset % 16
    d_blocks = torch.full((nb * N.BGZF_SLOT,), 0xAA, dtype=torch.uint8, device='cuda')
    d_sizes = torch.zeros(nb, dtype=torch.int32, device='cuda')
    d_packed = torch.full((bound + 16,), 0xAA, dtype=torch.uint8, device='cuda')
    total = ctypes.c_size_t(0)
    N.check(lib.kbbq_bgzf_deflate_dev(ctx.handle, N.ptr(d_text), n, block_bytes, N.ptr(d_blocks), N.ptr(d_sizes), N.ptr(d_packed),
                                      ctypes.byref(total)))
    packed = d_packed.cpu().numpy()
    sizes = d_sizes.cpu().numpy().astype(np.int64)
    assert int(sizes.sum()) == total.value <= bound and sizes.min() >= 27 and sizes.max() <= block_bytes + 31
    assert np.all(packed[total.value:] == 0xAA)
    slots = d_blocks.cpu().numpy().reshape(nb, N.BGZF_SLOT)
    ends = np.concatenate([[0], np.cumsum(sizes)])
    used = np.arange(N.BGZF_SLOT)[None, :] < sizes[:, None]
    assert np.array_equal(slots[used], packed[:total.value])          # row by row: the slots' blocks joined
    assert np.all(slots[np.arange(N.BGZF_SLOT)[None, :] >= ((sizes + 3) // 4 * 4)[:, None]] == 0xAA)
    assert ends[-1] == total.value
    return packed[:total.value].tobytes(), sizes


def run(text, block_bytes, grid, offset=0):
    """launch, verify, and the model's bytes; returns the decoded blocks"""
    packed, sizes = launch(text, block_bytes, offset)
    blocks = B.verify(text, block_bytes, packed, sizes)
    want, want_sizes, _ = B.deflate(text, block_bytes, grid=grid)
    if packed != want:
        at = np.concatenate([[0], np.cumsum(sizes)])
        wat = np.concatenate([[0], np.cumsum(want_sizes)])
        bad = [b for b in range(len(sizes)) if packed[at[b]:at[b + 1]] != want[wat[b]:wat[b + 1]]]
        raise AssertionError('blocks %s (of %d) are not the model\'s' % (bad[:8], len(sizes)))
    return blocks, packed, sizes


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks_of', ['CUs + 1', '2 * CUs + 3'])
def test_a_workgroup_codes_several_blocks(blocks_of):
    """Gap 1: more blocks than workgroups.  Blocks of 1101 bytes, 282,920 or 566,978 bytes of text on 256 CUs.  Block b + CUs is
    of another kind than block b, which the same workgroup coded before it: after a block that gave all 257 literal symbols a code
    comes one of a single byte value (two symbols, three lengths, at most three distances), after that a stored one, after that one
    of four letters; the last block is 37 bytes short.  Every block's bytes are those of the piece deflated alone (the model
    resets what the kernel must, and test_bgzf_model_host.py holds the model to that)."""
    n_cu = cus()
    nblocks = n_cu + 1 if blocks_of == 'CUs + 1' else 2 * n_cu + 3
    text = C.wg_text(nblocks, n_cu)
    blocks, packed, sizes = run(text, C.WG_BLOCK, n_cu)
    assert len(blocks) == nblocks > n_cu
    C.props_wg(blocks, n_cu)
    # three of the blocks once more, each as a launch of its own: the same bytes
    at = np.concatenate([[0], np.cumsum(sizes)])
    for b in (n_cu - 1, n_cu, nblocks - 1):
        alone, _ = launch(text[b * C.WG_BLOCK:(b + 1) * C.WG_BLOCK], C.WG_BLOCK)
        assert alone == packed[at[b]:at[b + 1]], b


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nblocks', [513, 1024, 1025])
def test_more_blocks_than_the_scan_has_threads(nblocks):
    """Gap 2: bz_scan_sizes with two and three sizes a thread.  Blocks of 101 bytes (51,723 to 103,435 bytes of text), stored ones
    of 132 bytes and coded ones of about 50 in no regular order; launch() checks that the packed bytes are the slots' blocks joined
    and that nothing is written behind them."""
    text = C.many_text(nblocks)
    blocks, packed, sizes = run(text, C.MANY_BLOCK, cus())
    assert len(blocks) == nblocks
    C.props_many(blocks, sizes)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_tokens_over_three_words():
    """Gap 3: bz_put's third word.  One block of 65,280 bytes (bgzf_cases.design_three_words): at least twenty tokens of 34 bits
    and more, the largest of at least 40, at least one of them across three words of the kernel's buffer."""
    blocks, _, _ = run(C.golden('three_words'), C.BLOCK, cus())
    rec = C.props_three_words(blocks)
    print('three-word tokens %d, largest token %d bits' % (rec['three_words'], rec['max_token_bits']))


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_the_code_length_code_is_limited_to_7_bits():
    """Gap 4: bz_build_code at limit = 7.  A block of 498 bytes, 128 byte values (bgzf_cases.CL_LIMIT_FREQ): one tile, so
    literals only; the counts of the code-length symbols, read from the GPU's header, give a tree 8 deep."""
    blocks, _, _ = run(C.cl_limit_text(), C.BLOCK, cus())
    assert C.props_cl_limit(blocks) == 8


def test_the_distance_code_is_limited_to_15_bits():
    """Gap 4: bz_build_code for the distances.  One block of 65,280 bytes (bgzf_cases.design_dist_limit), 4,180 matches over 17
    distance symbols with Fibonacci counts: a tree 16 deep, read from the GPU's tokens."""
    blocks, _, _ = run(C.golden('dist_limit'), C.BLOCK, cus())
    assert C.props_dist_limit(blocks) == 16


def test_the_literal_code_is_limited_to_15_bits():
    """Gap 4: bz_build_code for literals and lengths.  One block of 65,280 bytes (bgzf_cases.design_ll_limit) with exact counts:
    a tree 18 deep.  (The shuffled text of test_gpu_bgzf.py's sixth case is parsed into thousands of matches; the model shows its
    tree 13 deep, so that case limits nothing.)"""
    blocks, _, _ = run(C.golden('ll_limit'), C.BLOCK, cus())
    assert C.props_ll_limit(blocks) == 18


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_every_length_and_the_ends_of_every_distance_symbol():
    """Gap 5: 255 blocks of 771 bytes, block b with a match of 4 + b bytes at a distance of at most 512 (bgzf_cases.near_text),
    and one block of 65,280 bytes (design_far_bounds) with the lowest and the highest distance of the symbols 18 .. 29 and a match
    of 258 bytes that starts at position 511 of a tile.  Together: every length 4 .. 258, the lowest and the highest distance of
    every symbol (1 and 32768 among them), and 257 bytes carried into the next tile."""
    near, _, _ = run(C.near_text(), C.NEAR_BLOCK, cus())
    far, _, _ = run(C.golden('far_bounds'), C.BLOCK, cus())
    assert len(near) == 255
    C.props_bounds(near, far)


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 1, 7])
def test_crc_strips_and_both_copy_in_paths(offset):
    """Gap 6: 114 sizes (1 .. 64, either side of each of the 16 changes of the strip length, whole numbers of strips of 4 and 12
    bytes and a byte either side, 65,280), random bytes so that the block is stored and only the CRC and the copy of the text are
    at work; the text at a 16-byte boundary (16-byte loads and a tail) and 1 and 7 bytes behind one (byte loads)."""
    base = C.crc_base().tobytes()
    for n in C.crc_sizes():
        text = base[offset:offset + n]
        blocks, packed, _ = run(text, C.BLOCK, 1, offset)
        assert blocks[0]['btype'] == 0 and len(packed) == n + 31, n
