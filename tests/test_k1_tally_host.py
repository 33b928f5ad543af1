"""
CPU tests of tests/k1_tally.py, the NumPy reference and the restated launch plan that tests/test_gpu_k1_routes.py holds K1 to.

1. reference_tally equals the oracle (oracle.accumulate, itself pinned to the reference's goldens) wherever the oracle can be
   asked: the golden cases, sorted synthetic shapes, mate-pair and twins rows through their unpacked reads.
2. k1_plan gives the figures the project states for its own launch layer (csrc/kbbq_kernels_v3.h).
3. Discrimination: ten index mistakes, each applied to a copy of the reference, change the tables on every directed input
   where they can; EXEMPT lists the (mistake, input) pairs where they cannot, with the reason -- and is exact: a pair listed
   there that does differ fails the test too.
"""
import numpy as np
import pytest

import k1_tally as K
from conftest import GOLDEN_CASES, load_golden

TABLES = ['pos_errs', 'pos_total', 'dinuc_errs', 'dinuc_total']


def _same(got, want):
    for g, w, k in zip(got, want, TABLES):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), k


# ---- 1. the reference is the oracle's ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_reference_equals_goldens_and_oracle(oracle, name):
    info, gold = load_golden(name)
    c = info['case']
    seq, cseq, qual, meta = oracle.synth(0, c['n'], c['n'], c['seed'], c['len_lo'], c['len_hi'], c['nrg'], c['qlo'], c['qhi'])
    R, _, S2 = gold['pos_total'].shape
    got = K.reference_tally(seq, cseq, qual, meta, R, S2, 6)
    _same(got, [gold[k] for k in TABLES])
    _same(got, oracle.accumulate(seq, cseq, qual, meta, R, S2 // 2, minscore=6)[5:9])
    assert got[1].sum() > 0 and got[0].sum() > 0 and got[2].sum() > 0


@pytest.mark.parametrize('shape', [
    dict(n=65, len_lo=150, len_hi=150, nrg=3),
    dict(n=700, len_lo=1, len_hi=16, nrg=1),
    dict(n=900, len_lo=36, len_hi=300, nrg=5),
    dict(n=300, len_lo=100, len_hi=100, nrg=2, qlo=2, qhi=42),
])
@pytest.mark.parametrize('minscore', [0, 6, 20])
def test_reference_equals_oracle_on_sorted_synthetic_reads(oracle, shape, minscore):
    s = dict(first=0, total=shape['n'], seed=11 + shape['n'], qlo=0, qhi=41)
    s.update(shape)
    p = oracle.synth(**s)
    R, S = s['nrg'], s['len_hi']
    _same(K.reference_tally(*p, R, 2 * S, minscore), oracle.accumulate(*p, R, S, minscore=minscore)[5:9])


def test_reference_split_threshold_is_two_oracle_runs(oracle):
    """dinuc_minscore 20 above minscore 6: the cycle tables of a run at 6, the context tables of a run at 20."""
    p = oracle.synth(0, 900, 900, 3, 36, 300, 5, 0, 41)
    lo, hi = oracle.accumulate(*p, 5, 300, minscore=6)[5:9], oracle.accumulate(*p, 5, 300, minscore=20)[5:9]
    assert hi[3].sum() < lo[3].sum()
    _same(K.reference_tally(*p, 5, 600, 6, dinuc_minscore=20), (lo[0], lo[1], hi[2], hi[3]))
    _same(K.reference_tally(*p, 5, 600, 6, dinuc_minscore=3), lo)        # a lower context threshold changes nothing


def _pair_reads(S, rows, twins):
    """2 * rows reads of length S, neighbours sharing a read group: first / second in pair, or all first (twins)."""
    r = np.arange(2 * rows)
    return K.planes(np.full(2 * rows, S), 0 * r if twins else r & 1, 2 * ((r // 2 // 3 + r // 128) % 2), (S + 15) // 16 * 16,
                    base=lambda rr, at: K.DB[(at + 7 * rr) % 25], qual=lambda rr, at: (at * 3 + 5 * rr) % K.NQ,
                    err=lambda rr, at: (at + 3 * rr) % 7 == 0)


@pytest.mark.parametrize('twins', [False, True])
@pytest.mark.parametrize('S', [50, 150])
def test_reference_on_pair_rows_is_the_oracle_on_the_unpacked_reads(oracle, S, twins):
    p = _pair_reads(S, 64 + 5, twins)
    want = oracle.accumulate(*p, 3, S, minscore=6)[5:9]
    _same(K.reference_tally(*p, 3, 2 * S, 6), want)
    rows = K.pack_pairs(p, S)
    assert rows[0].shape[1] == K.pair_pitch(2 * S) and np.all(rows[0][:, S] == ord('N')) and not rows[2][:, S].any()
    _same(K.reference_tally(*rows, 3, 2 * S, 6, pairs=True, twins=twins), want)
    if not twins:                                       # ... and the two kinds of row differ where they must
        assert not np.array_equal(K.reference_tally(*rows, 3, 2 * S, 6, pairs=True, twins=True)[1], want[1])


def test_reference_takes_rows_in_any_order(oracle):
    """The oracle needs non-decreasing lengths; the reference gives the same tables for any order of the rows."""
    p = oracle.synth(0, 500, 500, 9, 36, 300, 3, 0, 41)
    want = oracle.accumulate(*p, 3, 300, minscore=6)[5:9]
    order = np.random.default_rng(1).permutation(500)
    assert (np.diff((p[3][order] & 0xFFFF).astype(np.int64)) < 0).any()
    with pytest.raises(IndexError):
        oracle.accumulate(*[a[order] for a in p], 3, 300, minscore=6)
    _same(K.reference_tally(*[a[order] for a in p], 3, 600, 6), want)


def test_reference_refuses_what_it_does_not_model():
    p = K.one_bin_reads(16, 16, 4, False)
    K.reference_tally(*p, 1, 32, 6)
    q = p[2].copy(); q[1, 3] = 33 + 43
    with pytest.raises(AssertionError):
        K.reference_tally(p[0], p[1], q, p[3], 1, 32, 6)
    s = p[0].copy(); s[2, 0] = ord('R')
    with pytest.raises(AssertionError):
        K.reference_tally(s, p[1], p[2], p[3], 1, 32, 6)
    s = p[0].copy(); s[2, 0] = ord('a')
    with pytest.raises(AssertionError):
        K.reference_tally(s, s, p[2], p[3], 1, 32, 6)


# ---- 2. the plan ------------------------------------------------------------------------------------------------------------------

def test_plan_gives_the_flush_iterations_the_kernel_header_states():
    """csrc/kbbq_kernels_v3.h: 6 iterations for 150-base reads one to a row (10 chunks), 3 for their mate-pair rows (19 chunks),
    4 for 13-chunk rows."""
    assert K.k1_plan(150, 160, 6, 0)['dn_flush_iters'] == 6
    assert K.k1_plan(150, 304, 6, 0, pairs=True, nib=True)['dn_flush_iters'] == 3
    assert K.k1_plan(100, 208, 6, 0, pairs=True, nib=True)['dn_flush_iters'] == 4
    assert K.k1_plan(150, 304, 6, 0, pairs=True, nib=True)['route'] == 'joint' == K.k1_plan(100, 208, 6, 0, pairs=True, nib=True)['route']
    assert K.k1_plan(150, 304, 6, 0, pairs=True, nib=True)['ntrash'] == 1 and K.k1_plan(100, 208, 6, 0, pairs=True, nib=True)['ntrash'] == 8
    # character mate-pair rows of the same widths are general forms with the same iterations
    assert K.k1_plan(150, 304, 6, 0, pairs=True)['route'] == 'v3' and K.k1_plan(150, 304, 6, 0, pairs=True)['dn_flush_iters'] == 3
    for cpr in range(1, 32):                             # a flush comes before a half can overflow, and not an iteration early
        p = K.k1_plan(16 * cpr, 16 * cpr, 6, 16 * cpr)
        if p['route'] == 'v3':
            assert p['copy_bound'] * p['dn_flush_iters'] <= 65535 < p['copy_bound'] * (p['dn_flush_iters'] + 1)


def test_plan_gives_the_first_generation_kernels_their_stated_shapes():
    """k1_accumulate holds the 43 x (2S | 1) table up to S = 459 (163,576 B of the 163,840); S = 460 needs column tiles."""
    a, b = K.k1_plan(459, 464, 6, 459), K.k1_plan(460, 464, 6, 460)
    assert (a['route'], a['lds']) == ('plain', 163576) and b['route'] == 'tiled'
    assert K.k1_plan(459, 464, 0, 0)['route'] == 'plain' and K.k1_plan(460, 464, 0, 0)['route'] == 'tiled'


def test_plan_ends_the_untrimmed_rows_where_the_project_says():
    """Attempt 0 (16 copies, rows of 3S words): up to S = 186 at minscore 6, up to S = 138 at minscore 0 -- 150-base reads on
    character planes at minscore 0 run trimmed rows or, with no promised shortest read, the first-generation kernel."""
    for minscore, last in ((6, 186), (0, 138)):
        for S in (last, last + 1):
            pitch = (S + 15) // 16 * 16
            p, q = K.k1_plan(S, pitch, minscore, 0), K.k1_plan(S, pitch, minscore, S)
            assert (p['route'] == 'v3') == (S == last)
            assert (q['route'], q['attempt']) == ('v3', 0 if S == last else 1)
    assert K.k1_plan(150, 160, 0, 0)['route'] == 'plain' and K.k1_plan(150, 160, 0, 100)['attempt'] == 1


def test_plan_of_2x50_mate_pair_rows():
    p = K.k1_plan(50, 112, 6, 0, pairs=True, nib=True)
    assert (p['route'], p['dn'], p['cut'], p['dn_flush_iters'], p['pos_copies']) == ('v3', 16, 0, 9, 2)
    assert p == K.k1_plan(50, 112, 6, 30, pairs=True)    # a promised shortest read trims no mate-pair row


# ---- 3. discrimination --------------------------------------------------------------------------------------------------------------

def _inputs():
    d = K.directed_reads(100, 36)
    K.check_directed(d, 100, 36)
    same = K.directed_reads(187, 187)
    K.check_directed(same, 187, 187)
    pr, tw = _pair_reads(50, 64 + 5, False), _pair_reads(50, 64 + 5, True)
    return {
        'directed': (d, dict(R=3, S2=200, minscore=6)),
        'directed_split': (d, dict(R=3, S2=200, minscore=6, dinuc_minscore=20)),
        'one_length': (same, dict(R=3, S2=374, minscore=6)),
        'pair_rows': (K.pack_pairs(pr, 50), dict(R=3, S2=100, minscore=6, pairs=True)),
        'twins_rows': (K.pack_pairs(tw, 50), dict(R=3, S2=100, minscore=6, pairs=True, twins=True)),
        'one_bin': (K.one_bin_reads(150, 160, 70, True), dict(R=2, S2=300, minscore=6)),
    }


INPUTS = ['directed', 'directed_split', 'one_length', 'pair_rows', 'twins_rows', 'one_bin']
NO_SPLIT = 'no context threshold above minscore'
ONE_BIN = 'every base is an A at quality 30 in a first-in-pair read of read group 0'
EXEMPT = {
    ('mirror_with_S', 'one_length'): 'every second-in-pair read has the tables\' length S',
    ('mirror_with_S', 'pair_rows'): 'both mates of a row have length S',
    ('mirror_with_S', 'twins_rows'): 'no second-in-pair read',
    ('mirror_off_by_one', 'twins_rows'): 'no second-in-pair read',
    ('second_ignored', 'twins_rows'): 'no second-in-pair read',
    ('split_on_cycle', 'directed'): NO_SPLIT, ('split_ignored', 'directed'): NO_SPLIT,
    ('split_on_cycle', 'one_length'): NO_SPLIT, ('split_ignored', 'one_length'): NO_SPLIT,
    ('split_on_cycle', 'pair_rows'): NO_SPLIT, ('split_ignored', 'pair_rows'): NO_SPLIT,
    ('split_on_cycle', 'twins_rows'): NO_SPLIT, ('split_ignored', 'twins_rows'): NO_SPLIT,
    ('split_on_cycle', 'one_bin'): NO_SPLIT, ('split_ignored', 'one_bin'): NO_SPLIT,
    ('mirror_off_by_one', 'one_bin'): ONE_BIN, ('mirror_with_S', 'one_bin'): ONE_BIN, ('second_ignored', 'one_bin'): ONE_BIN,
    ('read_group_ignored', 'one_bin'): ONE_BIN, ('N_is_a_context', 'one_bin'): ONE_BIN, ('gt_for_ge', 'one_bin'): ONE_BIN,
    ('prev_cur_swapped', 'one_bin'): ONE_BIN + ': the context AA is its own transpose',
}


@pytest.fixture(scope='module')
def inputs():
    out = _inputs()
    assert list(out) == INPUTS
    return {k: (p, kw, K.reference_tally(*p, **kw)) for k, (p, kw) in out.items()}


@pytest.mark.parametrize('mistake', K.MISTAKES)
def test_every_index_mistake_changes_the_tables(inputs, mistake):
    assert len(K.MISTAKES) >= 8 and all(m in K.MISTAKES and i in INPUTS and why for (m, i), why in EXEMPT.items())
    for name in INPUTS:
        p, kw, want = inputs[name]
        got = K.mistaken_tally(mistake, *p, **kw)
        differs = any(not np.array_equal(g, w) for g, w in zip(got, want))
        assert differs == ((mistake, name) not in EXEMPT), (mistake, name, EXEMPT.get((mistake, name)))
    # the mistakes about one table leave the other alone
    p, kw, want = inputs['directed_split']
    got = K.mistaken_tally(mistake, *p, **kw)
    if mistake in ('mirror_off_by_one', 'mirror_with_S', 'second_ignored', 'split_on_cycle'):
        assert np.array_equal(got[3], want[3]) and not np.array_equal(got[1], want[1])
    if mistake in ('first_base_context', 'prev_cur_swapped', 'N_is_a_context', 'split_ignored'):
        assert np.array_equal(got[1], want[1]) and not np.array_equal(got[3], want[3])
