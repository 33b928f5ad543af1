"""
The inputs of tests/test_gpu_aligned_edges.py can expose a miss: asserted from the CPU oracle alone (no GPU, no torch).
A kernel that drops a flag can only be caught where a flag is expected, and one that never writes a chunk only where that chunk
holds a flag -- these are the conditions the generator (tests/aligned_model.py) has to meet, with its fixed seeds.
"""
import numpy as np
import pytest

import aligned_model as AM


@pytest.fixture(scope='module')
def short():
    world = AM.short_world()
    return world, AM.short_families(world)


def test_the_site_mask_has_its_density_and_its_runs():
    for world in (AM.short_world(), AM.long_world()):
        assert 0.25 < world.mask.mean() < 0.36
        for want in (0, 1):
            edges = np.flatnonzero(np.diff(np.concatenate([[2], world.mask, [2]])))
            runs = np.diff(edges)[world.mask[edges[:-1]] == want]
            assert runs.max() >= 20, want
        assert set(np.unique(world.genome)) == set(b'ACGT')
        assert np.array_equal(world.fused & 0x7F, world.genome) and np.array_equal(world.fused >> 7, world.mask)


def test_every_family_is_there_and_both_flag_planes_are_dense(short):
    world, fams = short
    assert set(fams) == set(AM.FAMILIES)
    for name, reads in fams.items():
        assert len(reads) > 0, name
        assert {r.is_reverse for r in reads} == {False, True}, name
        assert min(r.reference_start for r in reads) == 0 and max(r.reference_end for r in reads) == world.G, name
        flags = [AM.expected(r, world) for r in reads]
        assert not any(isinstance(f, type) for f in flags), name           # none of these raises
        bases = sum(len(r) for r in reads)
        errors, skips = sum(int(e.sum()) for e, _ in flags), sum(int(s.sum()) for _, s in flags)
        assert errors > 0.10 * bases and skips > 0.10 * bases, (name, errors / bases, skips / bases)
        assert {len(r) for r in reads} <= set(AM.SHORT_N), name


def test_the_deletion_cases_hang_on_the_site_at_the_window_edge(short):
    """For dat + 1 + dlen = 15, 16 (the deletion's sites end inside / at the end of the target base's 16-byte window) and 17, 18
    (one / two sites outside it): a read whose mask is set on the LAST deleted site only, so that the target base's skip flag is
    that one site's."""
    world, fams = short
    seen = set()
    for r in fams['deletion']:
        ops = r.cigartuples
        if r.is_reverse or len(ops) != 3 or ops[1][0] != AM.D:
            continue
        edge, first = AM.deletion_window_edge(r)
        l = ops[1][1]
        sites = world.mask[first:first + l]
        if sites[-1] and not sites[:-1].any() and not world.mask[first - 1]:
            e, s = AM.expected(r, world)
            assert s[ops[0][1] - 1]                                       # ... and the oracle does skip the target base
            seen.add(edge)
    assert {15, 16, 17, 18} <= seen


def test_the_raising_shapes_raise_in_the_oracle(short):
    world, _ = short
    reads = AM.raising_reads(world)
    assert len(reads) >= 12
    classes = [AM.expected(r, world) for r in reads]
    assert all(c in (IndexError, ValueError) for c in classes), classes
    assert classes.count(IndexError) >= 4 and classes.count(ValueError) >= 4
    assert all(r.reference_end <= world.G for r in reads)


@pytest.mark.parametrize('n', AM.LONG_N)
def test_no_chunk_of_a_long_row_can_stay_unwritten_unnoticed(n):
    """Every complete 16-base output chunk with index >= 256 of every long-row case holds at least one expected flag."""
    world = AM.long_world()
    reads = AM.long_rows(world, n)
    names = {r.family.split('_', 2)[2] for r in reads}
    assert {'one_m', 'composed_deletion', 'composed_insertion', 'five_operations', 'many_operations'} <= names
    assert any(x.startswith('queued_256_') for x in names)
    many = [len(r.cigartuples) for r in reads if r.family.endswith('many_operations')]
    assert min(many) >= 100 and max(many) <= 400, many
    for r in reads:
        assert len(r) == n and 0 <= r.reference_start and r.reference_end <= world.G
        e, s = AM.expected(r, world)
        full = n // 16
        flagged = (e | s)[:16 * full].reshape(full, 16).any(1)
        assert flagged[256:].all(), (str(r)[:80], 256 + int(np.flatnonzero(~flagged[256:])[0]))
        assert e.mean() > 0.10 and s.mean() > 0.10
    # a queued chunk whose index needs more than eight bits, on either strand (forward: chunk c itself; reverse: the mirror of chunk 0)
    assert any(r.family.endswith('queued_256_7') and not r.is_reverse for r in reads) or n == 4097
    assert any(r.family.endswith('queued_0_7') and r.is_reverse for r in reads)


def test_the_mixed_batch_mixes():
    world = AM.long_world()
    lens = {len(r) for r in AM.mixed_rows(world)}
    assert lens == {37, 4113}


def test_the_canonical_restatement_on_a_read_worked_by_hand():
    """K6's rule on one forward and one reverse read, written out."""
    seq = np.zeros((2, 16), dtype=np.uint8); seq[:, :8] = np.frombuffer(b'ACGTNRAC', dtype=np.uint8)
    oq = np.zeros((2, 16), dtype=np.uint8); oq[:, :8] = 33 + np.array([10, 3, 10, 10, 10, 10, 10, 10])
    err = np.zeros((2, 16), dtype=np.uint8); err[:, 2] = 1
    skip = np.zeros((2, 16), dtype=np.uint8); skip[:, 3] = 1
    clip = np.array([1 | (8 << 16)] * 2, dtype=np.uint32)
    trim = np.array([7 | (8 << 16)] * 2, dtype=np.uint32)
    flags = np.array([0 | (2 << 16), 1 | 2 | (1 << 16)], dtype=np.uint32)
    s, q, e, meta = AM.canonical_reads(seq, oq, err, skip, clip, trim, flags, 8, 6)
    assert bytes(s[0]) == b'CGTNRAC' + b'N' * 9 and bytes(s[1]) == b'GTNNACG' + b'N' * 9
    assert list(q[0][:8]) == [0, 43, 0, 0, 43, 43, 0, 0] and list(q[1][:8]) == [0, 43, 43, 0, 0, 43, 0, 0]
    assert list(np.flatnonzero(e[0])) == [1] and list(np.flatnonzero(e[1])) == [5]
    assert list(meta) == [8 | (2 << 16), 8 | (1 << 16) | (1 << 31)]


def test_count_q_restatement():
    qual = np.array([[40, 41, 40, 35, 99, 99]], dtype=np.uint8)
    err = np.array([[0, 1, 1, 1, 1, 1]], dtype=np.uint8)
    skip = np.array([[0, 0, 0, 1, 0, 0]], dtype=np.uint8)
    t, e = AM.count_q(qual, err, skip, [4], 33)
    assert t[7] == 2 and t[8] == 1 and t.sum() == 3 and e[7] == 1 and e[8] == 1 and e.sum() == 2
