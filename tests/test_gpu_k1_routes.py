"""
GPU tests (-m gpu) of K1's GENERAL forms -- k1v3_accumulate<SPLIT, 16 | 8, NIB, 0>, k1v3_bands<SPLIT, NIB> and the
first-generation k1_accumulate / k1_accumulate_tiled (csrc/kbbq_hip.hip accumulate_rows, k1_geometry, k1_lds_plan;
csrc/kbbq_kernels_v3.h k1v3_body) -- on every route of the launch layer.  Every case compares all four count tables, exactly,
with tests/k1_tally.py reference_tally (a NumPy statement of the tally that takes rows in any order; tests/test_k1_tally_host.py
pins it to the oracle), and asserts BEFORE anything runs, from k1_tally.k1_plan, which form and LDS geometry its shape reaches.
The KJ = 19 / 13 forms have their own files (test_gpu_k1_joint_rows.py and its neighbours).

Directed reads (k1_tally.directed_reads / check_directed; 16 x 64 + 65 rows: one full workgroup iteration, a full block, a block
of one row): reads of length S and of length exactly s_min, first and second in pair, in lanes 0 and 63 of a block, in the
first and the last row; lengths in no sorted order; empty reads; every quality 0..42 at a first and at a last base; all 25
context slots, N included; an error at position 0 and at len - 1 of a second-in-pair read of length s_min -- word
S + 2 (S - len) + len - 1 = 3S - cut - 1, the LAST word of a trimmed cycle row --; read groups 0 and 2 mixed in every block
(the kernel compacts the lanes of its group), read group 1 empty.

The asserted plans, (minscore, S, s_min): route, attempt, copies of the context table, cut, trash rows, copies of the cycle
table, iterations between two flushes of the context table.  Attempt 0: 16 copies, rows of 3S words; 1: 16 copies, rows of
3S - cut words; 2: 8 copies and cut.

    minscore 6                                          minscore 0
    ( 16,   1)  v3 0  16    0  8  4  63                 ( 16,   1)  v3 0  16    0  8  4  63
    ( 40,  20)  v3 0  16    0  8  2  21                 ( 40,  20)  v3 0  16    0  8  2  21
    (100,  36)  v3 0  16    0  8  1   9                 ( 90,  36)  v3 0  16    0  8  1  10
    (150, 100)  v3 0  16    0  4  1   6                 (110,  60)  v3 0  16    0  4  1   9
    (170, 120)  v3 0  16    0  2  1   5                 (125,  80)  v3 0  16    0  2  1   7
    (186, 150)  v3 0  16    0  1  1   5   last of 0     (138, 100)  v3 0  16    0  1  1   7   last of 0
    (187, 187)  v3 1  16  187  8  1   5   first of 1    (139, 139)  v3 1  16  139  8  1   7   first of 1
    (230, 200)  v3 1  16  200  2  1   4                 (180, 150)  v3 1  16  150  2  1   5
    (265, 265)  v3 1  16  265  1  1   3                 (206, 206)  v3 1  16  206  1  1   4   last of 1
    (278, 278)  v3 1  16  278  1  1   3   last of 1     (207, 207)  v3 2   8  207  8  1   2   first of 2
    (279, 279)  v3 2   8  279  8  1   1   first of 2    (300, 280)  v3 2   8  280  2  1   1
    (300, 280)  v3 2   8  280  8  1   1                 (320, 300)  v3 2   8  300  1  1   1
    (320, 300)  v3 2   8  300  4  1   1                 (332, 332)  v3 2   8  332  1  1   1   last of 2
    (404, 404)  v3 2   8  404  1  1   1   last of 2     (333, 333)  plain
    (405, 405)  plain                                   (460, 400)  tiled (321 rows)
    (395, 375)  plain
    (460, 400)  tiled (321 rows)
    2 x 50 bp mate-pair / twins rows (pitch 112, 7 chunks, KJ = 0), both minscores: v3 0 16 0 8 {2 at 6, 1 at 0} 9

Every shape runs on character planes and, up to 320 bases, on 4-bit planes, as the rows come and grouped by read group, with
and without SPLIT (a context threshold of 20).  The first-generation kernels serve character planes that are not grouped only
(every other caller is told that its tables do not fit), so `plain` and `tiled` run there.

One workgroup past each flush: all reads in read group 0 of compute_units // 2 + 1 (one workgroup: launch_k1), one letter, one
quality, no errors or an error at every base; 1024 * min(dn_flush_iters, 48) + {1, 64} rows, and + 1024 rows (a whole further
iteration) where the bin's real load would overflow a half if the flush came an iteration late: S = 150 and the 8-copy shape.

Bands: mate-pair rows need count tables of exactly 2 x their read length, and a KJ form has reads of at most 151 bases, while 8
copies start at 279 bases (minscore 6) -- no single accumulate_bands call can hold both.  Two calls: bands that plan 8, 16 and
16 copies (all merged into k1v3_bands), and a KJ band (launched alone) beside two bands of 16 copies (merged).
"""
import numpy as np
import pytest

import k1_tally as K
from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

R = 3
SPLIT_AT = 20
# (minscore, S, s_min, route, attempt, dn, cut, ntrash, pos_copies, dn_flush_iters)
SHAPES = [
    (6, 16, 1, 'v3', 0, 16, 0, 8, 4, 63),
    (6, 40, 20, 'v3', 0, 16, 0, 8, 2, 21),
    (6, 100, 36, 'v3', 0, 16, 0, 8, 1, 9),
    (6, 150, 100, 'v3', 0, 16, 0, 4, 1, 6),
    (6, 170, 120, 'v3', 0, 16, 0, 2, 1, 5),
    (6, 186, 150, 'v3', 0, 16, 0, 1, 1, 5),
    (6, 187, 187, 'v3', 1, 16, 187, 8, 1, 5),
    (6, 230, 200, 'v3', 1, 16, 200, 2, 1, 4),
    (6, 265, 265, 'v3', 1, 16, 265, 1, 1, 3),
    (6, 278, 278, 'v3', 1, 16, 278, 1, 1, 3),
    (6, 279, 279, 'v3', 2, 8, 279, 8, 1, 1),
    (6, 300, 280, 'v3', 2, 8, 280, 8, 1, 1),
    (6, 320, 300, 'v3', 2, 8, 300, 4, 1, 1),
    (6, 404, 404, 'v3', 2, 8, 404, 1, 1, 1),
    (6, 405, 405, 'plain', None, 0, 0, 1, 1, 0),
    (6, 395, 375, 'plain', None, 0, 0, 1, 1, 0),
    (6, 460, 400, 'tiled', None, 0, 0, 1, 1, 0),
    (0, 16, 1, 'v3', 0, 16, 0, 8, 4, 63),
    (0, 40, 20, 'v3', 0, 16, 0, 8, 2, 21),
    (0, 90, 36, 'v3', 0, 16, 0, 8, 1, 10),
    (0, 110, 60, 'v3', 0, 16, 0, 4, 1, 9),
    (0, 125, 80, 'v3', 0, 16, 0, 2, 1, 7),
    (0, 138, 100, 'v3', 0, 16, 0, 1, 1, 7),
    (0, 139, 139, 'v3', 1, 16, 139, 8, 1, 7),
    (0, 180, 150, 'v3', 1, 16, 150, 2, 1, 5),
    (0, 206, 206, 'v3', 1, 16, 206, 1, 1, 4),
    (0, 207, 207, 'v3', 2, 8, 207, 8, 1, 2),
    (0, 300, 280, 'v3', 2, 8, 280, 2, 1, 1),
    (0, 320, 300, 'v3', 2, 8, 300, 1, 1, 1),
    (0, 332, 332, 'v3', 2, 8, 332, 1, 1, 1),
    (0, 333, 333, 'plain', None, 0, 0, 1, 1, 0),
    (0, 460, 400, 'tiled', None, 0, 0, 1, 1, 0),
]
LAYOUTS = ['chars', 'chars_grouped', 'nib', 'nib_grouped']
NIB_MAX = 320                                         # the longest read 4-bit planes are made for


def _pitch(S):
    return (S + 15) // 16 * 16


def _cases():
    for shape in SHAPES:
        S, route = shape[1], shape[3]
        for layout in LAYOUTS:
            if layout != 'chars' and route != 'v3':
                continue                              # the first-generation kernels serve ungrouped character planes only
            if layout.startswith('nib') and S > NIB_MAX:
                continue
            yield pytest.param(shape, layout, id='m%d-S%d-%s' % (shape[0], S, layout))


def test_the_shapes_reach_every_class_of_the_plan():
    """What the list above claims, from k1_plan alone (nothing runs on the device here)."""
    for minscore in (6, 0):
        plans = {}
        for ms, S, s_min, *want in SHAPES:
            if ms != minscore:
                continue
            p = K.k1_plan(S, _pitch(S), ms, s_min)
            assert [p[k] for k in ('route', 'attempt', 'dn', 'cut', 'ntrash', 'pos_copies', 'dn_flush_iters')] == want, (ms, S)
            plans[S, s_min] = p
        v3 = [p for p in plans.values() if p['route'] == 'v3']
        assert {p['route'] for p in plans.values()} == {'v3', 'plain', 'tiled'}
        assert {p['attempt'] for p in v3} == {0, 1, 2} and {p['dn'] for p in v3} == {16, 8}
        assert {p['ntrash'] for p in v3} == {8, 4, 2, 1} and {p['pos_copies'] for p in v3} == {4, 2, 1}
        # both sides of every boundary between two attempts, and of the one to the first-generation kernel
        by_S = sorted((S, p['attempt'] if p['route'] == 'v3' else 3) for (S, s_min), p in plans.items() if S == s_min)
        edges = [(a, b) for (Sa, a), (Sb, b) in zip(by_S, by_S[1:]) if Sb == Sa + 1 and b == a + 1]
        assert edges == [(1, 2), (2, 3)]
        last0 = {6: 186, 0: 138}[minscore]               # (run with a shorter s_min: the same attempt 0)
        assert any(S == last0 for S, _ in plans) and plans[last0 + 1, last0 + 1]['attempt'] == 1
        assert K.k1_plan(last0, _pitch(last0), minscore, last0)['attempt'] == 0
        for (S, s_min), p in plans.items():
            if p['route'] == 'v3' and p['attempt']:      # trimmed rows: the edge read's last base is the row's last word
                assert p['cut'] == s_min and S + 2 * (S - s_min) + s_min - 1 == 3 * S - p['cut'] - 1


# ---- the launches ---------------------------------------------------------------------------------------------------------------------

def _lay(dev, p, layout, groups=R, pairs=False):
    b = dev.ReadBatch.from_host(p[0], p[2], p[3], cseq=p[1])
    if layout == 'chars' and not pairs:
        return b
    if layout == 'chars_grouped' and not pairs:
        laid = dev.group_by_rg(b, groups)
    else:
        laid = dev.lay_out(b, groups if layout.endswith('grouped') else 1, packed=layout.startswith('nib'), pairs=pairs)
    assert laid.nib == layout.startswith('nib') and (laid.seg is not None) == layout.endswith('grouped')
    assert isinstance(laid, dev.PairBatch) == pairs
    return laid


def _tally(dev, laid, groups, S, minscore, dmin=None, s_min=0):
    t = dev.Tables(groups, 2 * S)
    dev.accumulate(laid, t, minscore, dinuc_minscore=dmin, s_band=0 if isinstance(laid, dev.PairBatch) else S, s_min=s_min)
    return t.to_host()


def _same(got, want, what=''):
    for g, w, k in zip(got, want, ('pos_errs', 'pos_total', 'dinuc_errs', 'dinuc_total')):
        assert g.dtype == np.int64 and g.shape == w.shape
        bad = np.argwhere(g != w)
        assert not len(bad), '%s %s: %d cells differ, first (rg, q, column) %s: %d for %d' % (
            what, k, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


_directed = {}


def _directed_case(S, s_min, minscore, dmin):
    """The directed reads of a shape and their reference tables: made once, shared by the layouts, never written to."""
    rows = 321 if S >= 460 else K.DIRECTED_ROWS
    if (S, s_min) not in _directed:
        p = K.directed_reads(S, s_min, rows=rows)
        K.check_directed(p, S, s_min)
        _directed[S, s_min] = (p, {})
    p, wants = _directed[S, s_min]
    if (minscore, dmin) not in wants:
        wants[minscore, dmin] = K.reference_tally(*p, R, 2 * S, minscore, dinuc_minscore=dmin)
    return p, wants[minscore, dmin]


# ---- 1. directed reads on every route ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,layout', _cases())
def test_directed_reads_on_every_route(dev, shape, layout):
    minscore, S, s_min, *want_plan = shape
    plan = K.k1_plan(S, _pitch(S), minscore, s_min, lds_bytes=_lds_bytes(dev))
    assert [plan[k] for k in ('route', 'attempt', 'dn', 'cut', 'ntrash', 'pos_copies', 'dn_flush_iters')] == want_plan
    p, want = _directed_case(S, s_min, minscore, None)
    # the edge read: errors at both ends of a second-in-pair read of length s_min, columns 2 s_min - 1 and s_min of read group
    # 0 or 2 at quality 30 -- in the LDS the words S + 2 (S - s_min) and 3S - s_min - 1
    e = K.EDGE_ROW
    rg = int(p[3][e] >> 16) & 0x7FFF
    assert want[0][rg, 30, 2 * s_min - 1] >= 1 and want[0][rg, 30, s_min] >= 1 and want[0][1].sum() == 0 == want[1][1].sum()
    assert want[1][:, :minscore].sum() == 0 and (minscore > 0 or want[1][:, 0].sum() > 0)
    laid = _lay(dev, p, layout)
    _same(_tally(dev, laid, R, S, minscore, s_min=s_min), want, 'plain threshold')
    p, split = _directed_case(S, s_min, minscore, SPLIT_AT)
    assert np.array_equal(split[1], want[1]) and 0 < split[3].sum() < want[3].sum()
    _same(_tally(dev, laid, R, S, minscore, dmin=SPLIT_AT, s_min=s_min), split, 'SPLIT')


def _lds_bytes(dev):
    """The LDS a workgroup may use on this device: what the plans of this file were restated for."""
    n = dev.context(None).lds_bytes
    assert n == 163840, 'the plans of this file are those of a 160 KB LDS'
    return n


# ---- 2. mate-pair and twins rows of 2 x 50 bp (7 chunks: KJ = 0) ------------------------------------------------------------------------

def _pair_reads(S, rows, twins):
    """2 * rows reads of length S: first / second in pair (or all first: twins), mates in one read group, groups 0 and 2 mixed
    in every block of rows; every quality at a first and a last base, all 25 contexts, errors at both ends of second mates."""
    r = np.arange(2 * rows)
    second = 0 * r if twins else r & 1
    p = K.planes(np.full(2 * rows, S), second, 2 * ((r // 2 // 3 + r // 128) % 2), _pitch(S),
                 base=lambda rr, at: K.DB[(at + 7 * rr) % 25],
                 qual=lambda rr, at: np.where(at == 0, rr % K.NQ, np.where(at == S - 1, (rr * 7 + 3) % K.NQ, (at * 3 + 5 * rr) % K.NQ)),
                 err=lambda rr, at: ((at + 3 * rr) % 7 == 0) | ((rr % 16 == 1) & ((at == 0) | (at == S - 1))))
    seq, cseq, qual, meta = p
    assert set(qual[:, 0] - 33) == set(range(K.NQ)) == set(qual[:, S - 1] - 33)
    odd = np.nonzero(r % 16 == 1)[0]
    assert np.all(seq[odd, 0] != cseq[odd, 0]) and np.all(seq[odd, S - 1] != cseq[odd, S - 1])
    return p


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('twins', [False, True], ids=['pairs', 'twins'])
@pytest.mark.parametrize('minscore', [6, 0])
def test_mate_pair_rows_of_seven_chunks(dev, minscore, twins, layout):
    S, rows = 50, K.DIRECTED_ROWS
    plan = K.k1_plan(S, K.pair_pitch(2 * S), minscore, 0, pairs=True, nib=layout.startswith('nib'), lds_bytes=_lds_bytes(dev))
    assert [plan[k] for k in ('route', 'attempt', 'dn', 'cut', 'ntrash', 'pos_copies', 'dn_flush_iters')] == \
        ['v3', 0, 16, 0, 8, 2 if minscore else 1, 9]
    p = _pair_reads(S, rows, twins)
    laid = _lay(dev, p, layout, pairs=True)
    assert laid.twins == twins and laid.pitch == 112 and laid.n == rows
    for dmin in (None, SPLIT_AT):
        want = K.reference_tally(*p, R, 2 * S, minscore, dinuc_minscore=dmin)
        assert (want[1][..., S:].sum() == 0) == twins and want[0].sum() > 0 and want[2].sum() > 0
        _same(_tally(dev, laid, R, S, minscore, dmin=dmin), want, 'dinuc_minscore %s' % dmin)
        if not laid.nib:                             # the rows themselves, read by the byte-offset rule of DESIGN section 2
            host = [laid.seq[:rows].cpu().numpy(), laid.cseq[:rows].cpu().numpy(), laid.qual[:rows].cpu().numpy(),
                    laid.meta[:rows].cpu().numpy().view(np.uint32)]
            if laid.perm is not None:
                assert sorted(laid.perm.cpu().numpy().tolist()) == list(range(rows))
            _same(K.reference_tally(*host, R, 2 * S, minscore, dinuc_minscore=dmin, pairs=True, twins=twins), want, 'rows')


# ---- 3. one workgroup past each flush ------------------------------------------------------------------------------------------------

# (S, pitch, s_min, pairs): 6 iterations; the cycle flush at 48 before the context flush at 63; 8 copies, 1 iteration; 9 iterations
FLUSH_SHAPES = {'S150': (150, 160, 0, False), 'S16': (16, 16, 0, False), 'S300_8copies': (300, 304, 280, False), '2x50': (50, 112, 0, True)}
# the rows after the flush: one row, a whole block -- and a whole further ITERATION where the single bin's real load (S - 1
# contexts a read, 1024 reads an iteration, spread over the copies) would overflow a half if the flush came one iteration late.
# It would not at pitch 16 (the flush of both tables at 48 iterations comes anyway) nor on 2 x 50 bp rows (10 iterations of
# 98 * 1024 / 16 = 6,272 counts a copy stay below 65,536: the bound 1024 * 7 the flush is planned for is not reached).
FLUSH_CASES = [(name, extra) for name in FLUSH_SHAPES for extra in (1, 64)] + [('S150', 1024), ('S300_8copies', 1024)]


@pytest.mark.parametrize('layout', ['chars', 'nib'])
@pytest.mark.parametrize('errors', [False, True], ids=['clean', 'all_errors'])
@pytest.mark.parametrize('name,extra', FLUSH_CASES, ids=['%s-%d' % c for c in FLUSH_CASES])
def test_one_workgroup_past_a_flush(dev, name, extra, errors, layout):
    """Every base an A at quality 30 in read group 0: all counts of a copy of the context table land in ONE bin, i.e. in one
    16-bit half of a word (both halves when every base is an error).  Tables of compute_units // 2 + 1 read groups give read
    group 0 a single workgroup (launch_k1: max(1, compute units / R) of them), which walks 1024 rows per iteration:
    1024 * min(dn_flush_iters, 48) rows are the last ones before its first flush, `extra` more make it go on after it."""
    S, pitch, s_min, pairs = FLUSH_SHAPES[name]
    groups = dev.context(None).compute_units // 2 + 1
    assert dev.context(None).compute_units // groups == 1
    plan = K.k1_plan(S, pitch, 6, s_min, pairs=pairs, nib=layout == 'nib', lds_bytes=_lds_bytes(dev))
    assert plan['route'] == 'v3' and plan['dn'] == (8 if S == 300 else 16)
    assert plan['dn_flush_iters'] == {150: 6, 16: 63, 300: 1, 50: 9}[S]
    # one more iteration without a flush could put more than 65,535 counts into a half; the iterations it does make cannot
    assert plan['copy_bound'] * (plan['dn_flush_iters'] + 1) > 65535 >= plan['copy_bound'] * plan['dn_flush_iters']
    iters = min(plan['dn_flush_iters'], K.FLUSH_ITERS)
    assert (iters == K.FLUSH_ITERS) == (S == 16)         # pitch 16: the flush of BOTH tables at 48 iterations comes first
    rows = K.ROWS_PER_ITER * iters + extra
    assert plan['flush_rows'] == rows - extra
    if extra == K.ROWS_PER_ITER:                         # a late flush WOULD overflow: the average copy alone gets this many counts
        assert (S - 1) * K.ROWS_PER_ITER // plan['dn'] * (iters + 1) > 65535 and iters == plan['dn_flush_iters']
    reads = 2 * rows if pairs else rows
    p = K.one_bin_reads(S, _pitch(S), reads, errors)
    if pairs:
        p[3][1::2] |= np.uint32(1 << 31)
    assert rows * pitch < 1 << 20 or extra == K.ROWS_PER_ITER      # a plane of the rows the kernel reads: under 1 MiB (1.1 with a further iteration)
    want = K.reference_tally(*p, groups, 2 * S, 6)
    laid = _lay(dev, p, layout, groups=1, pairs=pairs) if (pairs or layout == 'nib') else _lay(dev, p, 'chars')
    got = _tally(dev, laid, groups, S, 6, s_min=s_min)
    _same(got, want)
    # no count crossed into the other half, and all of them are where they belong
    assert got[1].sum() == S * reads and got[3].sum() == (S - 1) * reads == got[3][0, 30, 0]
    assert np.all(got[1][0, 30, :S] == (rows if not pairs else rows))
    if errors:
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[3])
    else:
        assert got[0].sum() == 0 and got[2].sum() == 0


# ---- 4. bands ------------------------------------------------------------------------------------------------------------------------------

def _band(dev, S, s_min, layout, rows=K.DIRECTED_ROWS):
    p = K.directed_reads(S, s_min, rows=rows)
    K.check_directed(p, S, s_min)
    assert p[0].shape[1] == _pitch(S)                    # every band at its own pitch
    return p, (_lay(dev, p, layout), S, s_min)


def _widen(p, pitch):
    """Planes padded to a common pitch (N / N / 0), for the reference of all bands' reads together."""
    out = []
    for a, fill in zip(p[:3], (ord('N'), ord('N'), 0)):
        w = np.full((a.shape[0], pitch), fill, dtype=np.uint8)
        w[:, :a.shape[1]] = a
        out.append(w)
    return out + [p[3]]


@pytest.mark.parametrize('which', ['8_16_16_copies', 'KJ_alone_16_16'])
def test_bands_in_one_call(dev, monkeypatch, which):
    """accumulate_bands over directed bands, compared with the reference of ALL reads together; again with KBBQ_K1_BANDS=0 (a
    launch per band).  Mate-pair rows need tables of exactly twice their read length, so the KJ band (2 x 150 bp on 4-bit
    planes: launched alone) cannot share a call with a band of 8 copies (279 bases and more): two sets of bands."""
    lds = _lds_bytes(dev)
    if which == '8_16_16_copies':
        S_all, specs, kj = 300, [(300, 280), (100, 36), (40, 20)], None
        want_dn = [8, 16, 16]
    else:
        S_all, specs, kj = 150, [(150, 100), (40, 20)], 150
        want_dn = [16, 16]
    assert [K.k1_plan(S, _pitch(S), 6, s_min, lds_bytes=lds)['dn'] for S, s_min in specs] == want_dn
    items, all_planes = [], []
    for S, s_min in specs:
        p, item = _band(dev, S, s_min, 'nib_grouped')
        items.append(item)
        all_planes.append(_widen(p, _pitch(S_all)))
    if kj:
        assert K.k1_plan(kj, K.pair_pitch(2 * kj), 6, 0, pairs=True, nib=True, lds_bytes=lds)['route'] == 'joint'
        pp = _pair_reads(kj, 3 * 64 + 5, False)
        laid = _lay(dev, pp, 'nib_grouped', pairs=True)
        assert laid.pitch == 16 * 19 and laid.errbit        # (the layout carries the error bit wherever it may: a KJ form)
        items.insert(1, (laid, 0, 0))
        all_planes.append(_widen(pp, _pitch(S_all)))
    together = [np.concatenate([b[i] for b in all_planes]) for i in range(4)]
    for dmin in (None, SPLIT_AT):
        want = K.reference_tally(*together, R, 2 * S_all, 6, dinuc_minscore=dmin)
        for merged in ('1', '0'):
            monkeypatch.setenv('KBBQ_K1_BANDS', merged)
            t = dev.Tables(R, 2 * S_all)
            dev.accumulate_bands(items, t, 6, dinuc_minscore=dmin)
            _same(t.to_host(), want, 'KBBQ_K1_BANDS=%s dinuc_minscore %s' % (merged, dmin))


# ---- 5. a read shorter than the promised s_min ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout', ['chars', 'nib_grouped'])
@pytest.mark.parametrize('S,s_min', [(230, 200), (300, 280)], ids=['16_copies', '8_copies'])
def test_a_read_shorter_than_promised_is_an_index_error(dev, S, s_min, layout):
    """Rows trimmed to 3S - s_min words hold no second-in-pair read shorter than s_min: such a read is reported (the error
    ST_INDEX maps to: IndexError), never counted at a word of another row.  The tables after the raise are not asserted."""
    plan = K.k1_plan(S, _pitch(S), 6, s_min, lds_bytes=_lds_bytes(dev))
    assert plan['route'] == 'v3' and plan['attempt'] >= 1 and plan['cut'] == s_min
    p = [a.copy() for a in K.directed_reads(S, s_min)]
    row = 64 * 9 + 17
    short = s_min - 1
    p[0][row, short:] = ord('N'); p[1][row, short:] = ord('N'); p[2][row, short:] = 0
    p[3][row] = (int(p[3][row]) & 0xFFFF0000) | short
    laid = _lay(dev, p, layout)
    t = dev.Tables(R, 2 * S)
    with pytest.raises(IndexError):
        dev.accumulate(laid, t, 6, s_band=S, s_min=s_min)
    # ... and the same rows with the promise kept (s_min - 1) are counted
    want = K.reference_tally(*p, R, 2 * S, 6)
    _same(_tally(dev, laid, R, S, 6, s_min=short), want)
