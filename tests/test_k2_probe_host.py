"""
CPU tests of tests/k2_probe.py, the probe models the GPU tests of K2 (test_gpu_k2_probe.py) rest on:
  * `reference_apply` is the oracle's apply on every probe, at the shapes and thresholds below;
  * `fast_range` is the flag `kbbq_build_lut` writes into the blob -- 0 for every probe, 2 one past either end of the byte
    range, 1 when an entry leaves int8 -- and the flag is per model row: a cell no read reaches sets it as well;
  * the probes discriminate: for each index mistake a kernel could make (k2_probe.MISTAKES) ONE probe changes EVERY
    counted base whose looked-up index the mistake alters.  This is a condition on the probes, not on any kernel.
"""
import ctypes

import numpy as np
import pytest

import k2_probe as P

N_READS = 400


def _flags(model, minscore):
    from kbbq import _native
    lib = _native.load()
    a = [np.ascontiguousarray(x, dtype=np.int64) for x in model]
    R, Qt, S2 = a[3].shape
    blob = np.zeros((lib.kbbq_lut_bytes(R, Qt, S2) + 7) // 8, dtype=np.int64).view(np.uint8)
    flags = ctypes.c_int(-1)
    _native.check(lib.kbbq_build_lut(R, Qt, S2, a[4].shape[2], minscore, *[_native.ptr(x) for x in a], _native.ptr(blob),
                                     ctypes.byref(flags)))
    return flags.value


@pytest.fixture(scope='module')
def batch():
    made = {}

    def get(S, R):
        if (S, R) not in made:
            seq, _, qual, meta = P.reads(S, R, N_READS, seed=7 * S + R, len_lo=S // 3)
            made[S, R] = (seq, qual, meta)
        return made[S, R]
    return get


def _models(R, S2, q):
    """Every probe, and the models outside the fast range (the changed cell in the middle of mate 1's columns)."""
    models = P.probes(R, S2)
    models['one past 0'] = P.one_past_low(R, S2, R - 1, q, 17)
    models['one past 255'] = P.one_past_high(R, S2, R - 1, q, 17)
    models['int8 misfit'] = P.int8_misfit(R, S2)
    return models


@pytest.mark.parametrize('minscore', [0, 6, 20])
@pytest.mark.parametrize('S', [50, 100, 150, 151])
@pytest.mark.parametrize('R', [1, 3, 8])
def test_reference_apply_is_the_oracle(oracle, batch, R, S, minscore):
    seq, qual, meta = batch(S, R)
    L = P.lookups(seq, qual, meta, 2 * S, minscore)
    for name, model in _models(R, 2 * S, 30).items():
        got = P.reference_apply(seq, qual, meta, *model, minscore=minscore)
        want = oracle.apply(seq, qual, meta, *model, minscore=minscore)          # raw values, 0 behind the reads
        assert np.array_equal(got[L.inside], want[L.inside].astype(np.int64) + 33), name
        assert not got[~L.inside].any() and not want[~L.inside].any(), name
        assert (got != qual)[L.counted].any(), name


@pytest.mark.parametrize('minscore', [0, 6, 20])
@pytest.mark.parametrize('R,S2', [(1, 300), (3, 200), (8, 300), (1, 600), (8, 100)])
def test_the_blob_flags_are_the_range_predicate(R, S2, minscore):
    for name, model in P.probes(R, S2).items():
        assert P.fast_range(model, minscore) == 0, name
        assert _flags(model, minscore) == 0, name
        cyc, ctx = P.entries(model)
        assert np.ptp(cyc) + np.ptp(ctx) > 0
    # both ends of the contract are reached, not merely approached
    cyc, ctx = P.entries(P.context_probe(R, S2))
    sums = cyc[:, :, :, None] + ctx[:, :, None, :] + 33
    assert ctx.min() == -128 and ctx.max() == 127 and sums.min() == 0 and sums.max() == 255
    cyc, ctx = P.entries(P.negative_cycle_probe(R, S2))
    assert cyc.max() < 0 and cyc.min() == -128 and ctx.min() >= 95 and (cyc.min(axis=2) + ctx.min(axis=2) + 33).min() == 0
    assert len(set(ctx[0, 0].tolist())) == P.D and ctx[..., 16].all()
    # one past either end, at a cell mate 1 reaches and at one no read of S2 / 4 bases reaches (the flag is per row)
    q = max(minscore, 30)
    for col in (17, S2 // 2):
        for model, want in ((P.one_past_low(R, S2, R - 1, q, col), 2), (P.one_past_high(R, S2, R - 1, q, col), 2)):
            assert P.fast_range(model, minscore) == want == _flags(model, minscore)
    model = P.int8_misfit(R, S2)
    cyc, ctx = P.entries(model)
    sums = cyc[:, :, :, None] + ctx[:, :, None, :] + 33
    assert sums.min() >= 0 and sums.max() <= 255 and cyc.min() > 127 and ctx.max() < 0
    assert P.fast_range(model, minscore) == 1 == _flags(model, minscore)
    # a row below the threshold is not served from the model: one past the range there changes nothing ...
    if minscore:
        assert P.fast_range(P.one_past_low(R, S2, 0, minscore - 1, 17), minscore) == 0 == _flags(P.one_past_low(R, S2, 0, minscore - 1, 17), minscore)


@pytest.mark.parametrize('S,R', [(150, 8), (100, 3), (151, 1), (50, 8)])
def test_every_mistake_is_seen_on_every_base_it_touches(batch, S, R):
    seq, qual, meta = batch(S, R)
    L = P.lookups(seq, qual, meta, 2 * S)
    true = (L.r, L.q, L.col, L.ctx)
    models = P.probes(R, 2 * S)
    right = {name: P.values(m, *true) for name, m in models.items()}
    for what, mistake in P.MISTAKES.items():
        wrong = mistake(L, R)
        touched = np.zeros(len(L.r), dtype=bool)
        for a, b in zip(true, wrong):
            touched |= a != b
        if what == 'read group + 1' and R == 1:
            assert not touched.any()
            continue
        assert touched.any(), what
        share = {name: float((P.values(m, *wrong) != right[name])[touched].mean()) for name, m in models.items()}
        assert max(share.values()) == 1.0, (what, share)
        # what the mistake leaves alone: diagonal dinucleotides under a transposition, bases without a context
        if what == 'context transposed':
            assert np.array_equal(~touched, (L.ctx == 16) | (L.ctx % 5 == 0))
        if what == 'no context':
            assert np.array_equal(~touched, L.ctx == 16)
        if what in ('mirror dropped', 'twins mapping for the mirror'):
            assert np.array_equal(touched, L.second == 1)
