"""tests/bgzf_model.py without a GPU: the token decoder against streams zlib wrote; the encoder model against zlib (verify())
on the texts of tests/test_gpu_bgzf.py and on every designed input of tests/test_gpu_bgzf_edges.py (tests/bgzf_cases.py), whose
path records must say what each case is for; and four wrong encoders (broken=), each of which verify() or a case's property
check must refuse -- the evidence that the GPU tests would notice a kernel wrong in that way."""
import gzip
import zlib

import numpy as np
import pytest

import bgzf_cases as C
import bgzf_model as B

CUS = 256                                                  # workgroups of the model where a case is about sharing them


def fastq_like(n, seed=3):
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        L = int(rng.integers(100, 151))
        seq = rng.choice(np.frombuffer(b'ACGTN', dtype=np.uint8), L, p=[.24, .25, .25, .24, .02]).tobytes()
        q = np.where(rng.random(L) < 0.7, ord('F'), rng.integers(35, 75, L)).astype(np.uint8).tobytes()
        out.append(b'@read.%d\n%s\n+\n%s\n' % (len(out), seq, q))
        size += len(out[-1])
    return b''.join(out)[:n]


# ---- the decoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level,strategy', [(1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                            (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY)])
@pytest.mark.parametrize('kind', ['fastq', 'random', 'mixed'])
def test_tokens_reads_what_zlib_wrote(level, strategy, kind):
    rnd = np.random.default_rng(5).integers(0, 256, 40000, dtype=np.uint8).tobytes()
    text = dict(fastq=fastq_like(150000), random=rnd, mixed=fastq_like(30000) + rnd + b'a' * 70000 + fastq_like(9, 1))[kind]
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    payload = z.compress(text) + z.flush()
    blocks, got = B.tokens(payload)
    assert got == text and blocks[-1]['final'] and (blocks[-1]['end'] + 7) >> 3 == len(payload)
    types = {blk['btype'] for blk in blocks}
    coded = 1 if strategy == zlib.Z_FIXED else 2
    assert types == {coded} if kind == 'fastq' else types <= {0, coded}  # zlib stores what no code makes smaller
    replay = bytearray()                                   # the token list alone gives the text back, stored blocks apart
    for blk in blocks:
        assert blk['first'] == len(replay)
        if blk['btype'] == 0:
            replay += got[blk['first']:blk['first'] + blk['stored']]
            continue
        at = None
        for off, bits, t in blk['tokens']:
            assert at is None or off == at                  # tokens follow each other without a gap
            at = off + bits
            if isinstance(t, tuple):
                assert 3 <= t[0] <= 258 and 1 <= t[1] <= 32768
                for _ in range(t[0]):
                    replay.append(replay[-t[1]])
            else:
                replay.append(t)
        assert blk['eob'] == at or not blk['tokens']
        if strategy == zlib.Z_HUFFMAN_ONLY:
            assert not any(isinstance(t, tuple) for _, _, t in blk['tokens'])
    assert bytes(replay) == text


def test_tokens_refuses_damage():
    member = B.deflate_block(fastq_like(3000))[0]
    payload = bytearray(member[18:-8])
    assert B.tokens(bytes(payload))[1] == fastq_like(3000)
    with pytest.raises(ValueError):
        B.tokens(bytes(payload[:len(payload) // 2]))       # the stream ends inside the block
    payload[0] |= 6
    with pytest.raises(ValueError):
        B.tokens(bytes(payload))                            # BTYPE 3


# ---- the model -----------------------------------------------------------------------------------------------------------
def test_crc_by_strips_is_the_crc():
    base = C.crc_base().tobytes()
    for n in C.crc_sizes():
        assert B.crc32_strips(base[:n]) == zlib.crc32(base[:n]), n
    lengths = {B.strip_length(n) for n in C.crc_sizes()}
    assert lengths == set(range(4, 133, 8)) and all(L % 8 == 4 for L in lengths)   # an odd number of words, 17 lengths


@pytest.mark.parametrize('case', C.existing_texts(), ids=lambda c: c[0])
def test_model_on_the_texts_of_the_gpu_cases(case):
    name, text, bb = case
    packed, sizes, recs = B.deflate(text, bb, grid=CUS)
    blocks = B.verify(text, bb, packed, sizes)
    for blk, rec in zip(blocks, recs):
        assert blk['btype'] == rec['btype']
        if rec['coded']:                                   # the record agrees with what the decoder sees in the block
            seen = B.paths(blk)
            assert (seen['max_token_bits'], seen['three_words'], seen['max_carry']) == \
                   (rec['max_token_bits'], rec['three_words'], rec['max_carry'])
            assert seen['pairs'] == rec['pairs'] and blk['header_bits'] == rec['header_bits']
            assert not rec['lone_cl']                      # bz_plan_header's `used == 1`: not reachable, see its comment
    if name == 'random':
        assert [r['btype'] for r in recs] == [0]
    if name == '15 bits':                                  # the shuffled text is full of matches, its counts are not the ones designed and
        assert recs[0]['depth']['ll'] <= 15 and len(recs[0]['pairs']) > 1000   # nothing is limited: bgzf_cases.design_ll_limit does that
    if name == '32768':
        assert 32768 in recs[0]['dists'] and max(recs[0]['dists']) == 32768
    if name == 'equal bytes':
        assert recs[0]['lengths'] == {258} | {(B.BLOCK_MAX - 512) % 258} and recs[0]['max_carry'] > 0


@pytest.fixture(scope='module')
def designed():
    """name -> (text, block_bytes, model's packed bytes, sizes, records, decoded blocks)"""
    out = {}
    texts = dict(wg257=(C.wg_text(CUS + 1, CUS), C.WG_BLOCK), wg515=(C.wg_text(2 * CUS + 3, CUS), C.WG_BLOCK),
                 many513=(C.many_text(513), C.MANY_BLOCK), many1024=(C.many_text(1024), C.MANY_BLOCK),
                 many1025=(C.many_text(1025), C.MANY_BLOCK), three_words=(C.golden('three_words'), C.BLOCK),
                 cl_limit=(C.cl_limit_text(), C.BLOCK), ll_limit=(C.golden('ll_limit'), C.BLOCK), dist_limit=(C.golden('dist_limit'), C.BLOCK),
                 near=(C.near_text(), C.NEAR_BLOCK), far_bounds=(C.golden('far_bounds'), C.BLOCK))
    for name, (text, bb) in texts.items():
        packed, sizes, recs = B.deflate(text, bb, grid=CUS)
        out[name] = (text, bb, packed, sizes, recs, B.verify(text, bb, packed, sizes))
    return out


def check_designed(name, text, bb, packed, sizes, blocks=None):
    """verify() and the case's own property, as tests/test_gpu_bgzf_edges.py asks them of the GPU's bytes"""
    blocks = blocks or B.verify(text, bb, packed, sizes)
    if name.startswith('wg'):
        C.props_wg(blocks, CUS)
    if name == 'wg257':
        at = 0
        for b, size in enumerate(int(x) for x in sizes):  # every block equals its piece deflated alone
            assert packed[at:at + size] == B.deflate_block(text[b * bb:(b + 1) * bb])[0], b
            at += size
    elif name.startswith('many'):
        C.props_many(blocks, sizes)
    elif name in ('three_words', 'cl_limit', 'll_limit', 'dist_limit'):
        getattr(C, 'props_' + name)(blocks)
    return blocks


def test_the_stored_blocks_are_the_designs():
    for name, design in C.GOLDEN.items():
        assert C.golden(name) == design(), name             # python tests/bgzf_cases.py writes them again


def test_designed_inputs_take_their_paths(designed):
    for name, (text, bb, packed, sizes, recs, blocks) in designed.items():
        check_designed(name, text, bb, packed, sizes, blocks)
    C.props_bounds(designed['near'][5], designed['far_bounds'][5])
    assert len(designed['wg515'][4]) == 2 * CUS + 3 and designed['wg515'][4][-1]['n'] == C.WG_BLOCK - 37
    for name in ('wg257', 'wg515'):                        # unaligned block starts: both copy-in paths of the kernel
        assert {(b * C.WG_BLOCK) % 16 for b in range(len(designed[name][4]))} == set(range(16))
    rec = designed['three_words'][4][0]
    assert rec['three_words'] >= 1 and rec['max_token_bits'] >= 40 and rec['long_tokens'] >= 20
    rec = designed['cl_limit'][4][0]
    assert rec['n'] <= 512 and rec['limited'] == dict(ll=False, d=False, cl=True) and rec['depth']['cl'] == 8 and not rec['pairs']
    rec = designed['ll_limit'][4][0]
    assert rec['limited'] == dict(ll=True, d=False, cl=False) and rec['depth']['ll'] == 18
    rec = designed['dist_limit'][4][0]
    assert rec['limited'] == dict(ll=False, d=True, cl=False) and rec['depth']['d'] == 16
    rec = designed['far_bounds'][4][0]
    assert rec['max_carry'] == 257 and (258, 1022) in rec['pairs']
    assert all(C.near_pair(b) in r['pairs'] for b, r in enumerate(designed['near'][4]))
    for name in ('many513', 'many1024', 'many1025'):
        assert len(designed[name][4]) == int(name[4:]) and {r['btype'] for r in designed[name][4]} == {0, 2}


def test_crc_texts_are_stored():
    base = C.crc_base().tobytes()
    for n in C.crc_sizes():
        for off in (0, 1, 7):
            member, rec = B.deflate_block(base[off:off + n])
            assert rec['btype'] == 0 and len(member) == n + 31
            if n in (1, 64, 2049, C.BLOCK):
                B.verify(base[off:off + n], C.BLOCK, member, [len(member)])


# ---- the checker bites ---------------------------------------------------------------------------------------------------
CAUGHT_BY = dict(third_word='three_words', stale_lengths='wg257', no_repair_7='cl_limit', crc_shift='far_bounds')


@pytest.mark.parametrize('broken', B.BROKEN)
def test_a_wrong_encoder_is_refused(designed, broken):
    assert set(CAUGHT_BY) == set(B.BROKEN)
    name = CAUGHT_BY[broken]
    text, bb, good = designed[name][:3]
    packed, sizes, _ = B.deflate(text, bb, grid=CUS, broken=broken)
    assert packed != good
    with pytest.raises((AssertionError, ValueError, zlib.error, gzip.BadGzipFile)):
        check_designed(name, text, bb, packed, sizes)
    check_designed(name, text, bb, good, designed[name][3])  # ... and the same check passes the unbroken model


def test_wrong_encoders_differ_only_where_their_path_is_entered(designed):
    """Each variant leaves alone the inputs that do not enter its path: what catches it is the designed input, not luck."""
    text = fastq_like(3 * 4096)
    good = B.deflate(text, 4096, grid=CUS)[0]
    for broken in ('stale_lengths', 'no_repair_7'):        # three blocks, three workgroups; no code-length code over 7 bits
        assert B.deflate(text, 4096, grid=CUS, broken=broken)[0] == good
    assert B.deflate(text, 4096, grid=1, broken='stale_lengths')[0] != good
    small = fastq_like(4)                                  # one strip: nothing to shift
    assert B.deflate_block(small, broken='crc_shift')[0] == B.deflate_block(small)[0]
    text, bb, good = designed['dist_limit'][:3]            # no token of more than 29 bits
    assert B.deflate(text, bb, broken='third_word')[0] == good
