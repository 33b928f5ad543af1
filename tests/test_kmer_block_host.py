"""kmer.count_block without a device: the table is a Counter, the filter a record of what was asked of it, and every step writes
its name into one log.  What is checked is the block's own work -- the order of the steps, the sizes and budgets it hands on (the
numbers below are worked out by hand from the rules in kmer's module docstring), the info it returns and what it closes when a
step raises -- for the prefilter on and off, partitions 1, 3 and 'auto' (resolving to 1 and to more), both budget rules, and a
k-mer set in the count's place."""
import collections
import contextlib

import numpy as np
import pytest

# 17 keys: 6 seen once, 3 twice, 1 three times, 2 four times, 5 nine times.  h[2] = 3 > h[3] = 1 <= h[4] = 2: the valley is 3.
COUNTS = [1] * 6 + [2] * 3 + [3] + [4] * 2 + [9] * 5
T, KEPT = 3, 11                       # keep = 2 without min_count: 11 pairs are kept, whatever the number of rounds
W, ADMITTED, BITS = 100000, 60000, 4  # windows; what the filter admits; bits a window
WORDS = 8192                          # 8192 x 64 = 524,288 >= 4 x 100,000 > 4096 x 64: 131,072 bytes, 65,536 once `seen` is gone
R = 1000000                           # bytes of resident planes
M8, M2 = 8388608, 2097152             # KBBQ_DEVICE_BUDGET

# (prefilter, partitions, budget, resident) -> (P, slots, the budget the rounds and the solid table are given).  By hand:
# a table for n keys has the first power of two >= 2 n slots (from 1024) of 12 bytes; a partition of P is sized for
# ceil(9 n / 8 P) keys within HALF the budget; 'auto' is the first P whose uncapped table fits half the budget.
# room = budget - R, less the 65,536 bytes of `twice`: 7,388,608 / 7,323,072 of 8 MiB and 1,097,152 / 1,031,616 of 2 MiB.
CASES = {
    # no filter: 100,000 keys want 2^18 slots = 3,145,728 bytes, which half of 8 MiB (and of 7,388,608) holds
    (False, 1, M8, None): (1, 262144, M8), (False, 1, M8, R): (1, 262144, 7388608),
    (False, 'auto', M8, None): (1, 262144, M8), (False, 'auto', M8, R): (1, 262144, 7388608),
    # P = 3: ceil(900,000 / 24) = 37,500 keys -> 2^17
    (False, 3, M8, None): (3, 131072, M8), (False, 3, M8, R): (3, 131072, 7388608),
    # half of 2 MiB = 1,048,576 holds 2^16 slots (786,432): 32,768 keys.  112,500 / P <= 32,768 from P = 4 (28,125)
    (False, 'auto', M2, None): (4, 65536, M2),
    # half of 1,097,152 = 548,576 holds 2^15 slots (393,216): 16,384 keys.  112,500 / P <= 16,384 from P = 7 (16,072)
    (False, 'auto', M2, R): (7, 32768, 1097152),
    # the filter: 60,000 admitted keys want 2^17 slots = 1,572,864 bytes
    (True, 1, M8, None): (1, 131072, M8), (True, 1, M8, R): (1, 131072, 7323072),
    (True, 'auto', M8, None): (1, 131072, M8), (True, 'auto', M8, R): (1, 131072, 7323072),
    # P = 3: ceil(540,000 / 24) = 22,500 keys -> 2^16
    (True, 3, M8, None): (3, 65536, M8), (True, 3, M8, R): (3, 65536, 7323072),
    # the whole 2 MiB, the filter NOT taken off: 67,500 / P <= 32,768 from P = 3 (22,500; P = 2: 33,750)
    (True, 'auto', M2, None): (3, 65536, M2),
    # half of 1,031,616 = 515,808 holds 2^15 slots: 67,500 / P <= 16,384 from P = 5 (13,500; P = 4: 16,875)
    (True, 'auto', M2, R): (5, 32768, 1031616),
}


class Boom(Exception):
    pass


class World:
    """The stand-ins and their log.  fail = (event name, n): the n-th such event raises self.boom instead of happening."""

    def __init__(self, monkeypatch, budget, fail=None):
        from kbbq import kmer
        self.log, self.tables, self.filters, self.fail, self.boom, self.seen = [], [], [], fail, Boom('on purpose'), collections.Counter()
        self.given = {}                              # what load_set and count_partitioned were handed
        world = self

        class Table(collections.Counter):
            def __init__(self, k, slots):
                super().__init__()
                world.event('table', slots)
                self.k, self.slots, self.nbytes, self.closed = k, slots, 12 * slots, 0
                world.tables.append(self)

            def clear(self):
                world.event('clear')
                super().clear()

            def close(self):
                world.event('table.close')
                self.closed += 1

        class Filter:
            admitted = ADMITTED

            def __init__(self, words):
                world.event('filter', words)
                self.words, self.seen, self.closed = words, True, 0
                world.filters.append(self)

            @property
            def nbytes(self):
                return self.words * (16 if self.seen else 8)

            def release_seen(self):
                world.event('release_seen')
                self.seen = False

            def close(self):
                world.event('filter.close')
                self.closed += 1

        def histogram(table):
            world.event('hist')
            h = np.zeros(kmer.HIST, dtype=np.int64)
            for c in table.values():
                h[min(c, 256)] += 1
            return h

        def select(table, nbuckets, keep):
            world.event('select')
            pairs = sorted((key, c) for key, c in table.items() if c >= keep)
            return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int32), None

        def merge(table, keys, counts):
            world.event('merge')
            table.update(dict(zip(keys.tolist(), counts.tolist())))
            return table

        def load_set(path, min_count=None, slots=None, k=None, budget=None, slab=None):
            world.event('load')
            world.given['load'] = dict(path=path, min_count=min_count, slots=slots, k=k, budget=budget)
            table = Table(21, slots or 1024)
            return table, np.arange(kmer.HIST), 5, dict(k=21, kmers_from=path, loaded_kmers=7, slots=table.slots, table_bytes=table.nbytes)
        partitioned = kmer.count_partitioned

        def count_partitioned(count_round, k, P, slots, min_count, budget):
            world.given['partitioned'] = dict(P=P, slots=slots, budget=budget)
            return partitioned(count_round, k, P, slots, min_count, budget)
        for name, stand_in in (('KmerTable', Table), ('KmerFilter', Filter), ('kmer_histogram', histogram), ('select', select),
                               ('merge', merge), ('load_set', load_set), ('count_partitioned', count_partitioned)):
            monkeypatch.setattr(kmer, name, stand_in)

        def never(*a, **kw):
            raise AssertionError('a device call')
        monkeypatch.setattr(kmer, '_ctx', never)
        monkeypatch.setenv('KBBQ_DEVICE_BUDGET', str(budget))

    def event(self, name, *more):
        self.seen[name] += 1
        if self.fail == (name, self.seen[name]):
            raise self.boom
        self.log.append((name,) + more if more else name)

    def read(self, what, filter=None, table=None, parts=1, part=0):
        """One pass over the 17 keys: behind the filter only those seen twice or more are counted."""
        if what == 'prefilter':
            assert filter.seen and table is None
            return self.event('prefilter')
        self.event('count', parts, part)
        assert filter is None or not filter.seen
        for key, c in enumerate(COUNTS):
            if key % parts == part and (filter is None or c >= 2):
                table[key] += c

    @contextlib.contextmanager
    def stage(self, name, sync=False):
        assert sync is True
        self.log.append('<' + name)
        yield
        self.log.append(name + '>')


def _steps(prefilter, P, slots, staged=False):
    """The order the module docstring gives: filter, pass, release, table, the rounds (cleared before every round but the first),
    and the filter closed before the histogram of one round, after the last of several."""
    pre = [('filter', WORDS), 'prefilter', 'release_seen'] if prefilter else []
    if staged and prefilter:
        pre = ['<k-mer prefilter'] + pre + ['k-mer prefilter>']
    closed = ['filter.close'] if prefilter else []
    if P == 1:
        count = [('table', slots), ('count', 1, 0)]
        return pre + (['<k-mer count'] + count + ['k-mer count>'] if staged else count) + closed + ['hist']
    count = [('table', slots)]
    for p in range(P):
        count += (['clear'] if p else []) + [('count', P, p), 'hist', 'select']
    kept = sum(1 for p in range(P) if any(c >= 2 for key, c in enumerate(COUNTS) if key % P == p))
    count += ['table.close', ('table', 1024)] + ['merge'] * kept              # 11 pairs: the smallest table
    return pre + (['<k-mer count'] + count + ['k-mer count>'] if staged else count) + closed


@pytest.mark.parametrize('staged', (False, True))
@pytest.mark.parametrize('prefilter, partitions, budget, resident', sorted(CASES, key=str))
def test_the_steps_their_order_and_their_numbers(monkeypatch, prefilter, partitions, budget, resident, staged):
    from kbbq import kmer
    P, slots, within = CASES[prefilter, partitions, budget, resident]
    w = World(monkeypatch, budget)
    table, hist, t, info = kmer.count_block(w.read, W, 21, prefilter=prefilter, filter_bits=BITS, partitions=partitions,
                                            room=None if resident is None else budget - resident,
                                            **(dict(stage=w.stage) if staged else {}))
    assert w.log == _steps(prefilter, P, slots, staged)
    assert t == T and [int(hist[c]) for c in (2, 3, 4, 9)] == [3, 1, 2, 5] and int(hist[1]) == (0 if prefilter else 6)
    assert int(hist.sum()) == (11 if prefilter else 17)
    want = dict(slots=slots, table_bytes=12 * slots, filter_bytes=16 * WORDS if prefilter else 0, admitted=ADMITTED if prefilter else None)
    if P > 1:
        want.update(partitions=P, kept_pairs=KEPT, solid_slots=1024)
        assert w.given['partitioned'] == dict(P=P, slots=slots, budget=within)
        assert table is w.tables[1] and table.slots == 1024 and dict(table) == {key: c for key, c in enumerate(COUNTS) if c >= 2}
    else:
        assert 'partitioned' not in w.given and table is w.tables[0]
        assert dict(table) == {key: c for key, c in enumerate(COUNTS) if c >= 2 or not prefilter}
    assert info == want
    # the caller owns the table it is handed; everything else is closed, once
    assert table.closed == 0 and [x.closed for x in w.tables if x is not table] == [1] * (len(w.tables) - 1)
    assert [f.closed for f in w.filters] == ([1] if prefilter else [])


def test_slots_and_min_count_as_given(monkeypatch):
    from kbbq import kmer
    w = World(monkeypatch, M8)
    table, hist, t, info = kmer.count_block(w.read, W, 21, min_count=4, slots=2048, prefilter=True, partitions=2, room=M8 - R)
    # keep = min_count = 4: 7 pairs; the rounds' budget is what is left beside the planes and `twice`
    assert (t, info['slots'], info['kept_pairs'], info['partitions']) == (4, 2048, 7, 2)
    assert w.given['partitioned'] == dict(P=2, slots=2048, budget=M8 - R - 8 * WORDS)
    w = World(monkeypatch, M8)
    table, hist, t, info = kmer.count_block(w.read, W, 21, min_count=2, slots=4096)
    assert (t, info) == (2, dict(slots=4096, table_bytes=49152, filter_bytes=0, admitted=None)) and w.log == _steps(False, 1, 4096)


@pytest.mark.parametrize('min_count, P', ((0, 1), (0, 3), (-2, 1)))
def test_min_count_below_one(monkeypatch, min_count, P):
    """In one round after the count, as correct_reads always refused it; in several before the first table."""
    from kbbq import kmer
    w = World(monkeypatch, M8)
    with pytest.raises(ValueError, match=r'^min_count must be >= 1, got %d$' % min_count):
        kmer.count_block(w.read, W, 21, min_count=min_count, partitions=P)
    assert [x.closed for x in w.tables] == ([1] if P == 1 else [])


@pytest.mark.parametrize('resident', (None, R))
def test_a_set_in_the_place_of_the_count(monkeypatch, resident):
    from kbbq import kmer
    w = World(monkeypatch, M8)

    def read(*a, **kw):
        raise AssertionError('nothing is counted')
    table, hist, t, info = kmer.count_block(read, 0, None, min_count=6, slots=4096, kmers_from='x.set',
                                            room=None if resident is None else M8 - resident, stage=w.stage)
    assert w.log == ['<k-mer load', 'load', ('table', 4096), 'k-mer load>'] and table is w.tables[0] and table.closed == 0
    # correct_reads' rule leaves the budget to load_set; beside resident planes it is what they leave
    assert w.given['load'] == dict(path='x.set', min_count=6, slots=4096, k=None, budget=None if resident is None else 7388608)
    assert t == 5 and info == dict(k=21, kmers_from='x.set', loaded_kmers=7, slots=4096, table_bytes=49152, filter_bytes=0, admitted=None)
    w = World(monkeypatch, M8, fail=('load', 1))
    with pytest.raises(Boom) as caught:
        kmer.count_block(read, 0, None, kmers_from='x.set')
    assert caught.value is w.boom and w.tables == []


FAILURES = [(pre, P, step) for pre in (False, True) for P in (1, 3)
            for step in ([('filter', 1), ('prefilter', 1), ('release_seen', 1)] if pre else []) + [('table', 1), ('count', 1), ('hist', 1)]
            + ([('count', 2), ('clear', 2), ('hist', 3), ('select', 1), ('select', 3), ('table', 2), ('merge', 1), ('merge', 2)] if P > 1 else [])]


@pytest.mark.parametrize('prefilter, P, step', FAILURES)
def test_a_step_that_raises_closes_everything_once(monkeypatch, prefilter, P, step):
    from kbbq import kmer
    w = World(monkeypatch, M8, fail=step)
    with pytest.raises(Boom) as caught:
        kmer.count_block(w.read, W, 21, prefilter=prefilter, partitions=P, room=M8 - R)
    assert caught.value is w.boom                                    # unchanged, not wrapped
    assert [x.closed for x in w.tables] == [1] * len(w.tables) and [f.closed for f in w.filters] == [1] * len(w.filters)


def test_no_valley_closes_the_table_and_keeps_its_text(monkeypatch):
    from kbbq import kmer
    w = World(monkeypatch, M8)
    monkeypatch.setattr(kmer, 'kmer_histogram', lambda table: np.arange(kmer.HIST, 0, -1))
    with pytest.raises(ValueError, match=r'^the k-mer count histogram has no valley in 2\.\.255: give min_count$'):
        kmer.count_block(w.read, W, 21)
    assert [x.closed for x in w.tables] == [1]


def test_count_rounds_is_the_first_half(monkeypatch):
    """`kbbq count`'s use: one round clears nothing and keeps from `keep` up; count_plan sizes its table by correct_reads' rule."""
    from kbbq import kmer
    w = World(monkeypatch, M2)
    filt, admitted, filter_bytes, P, slots, budget = kmer.count_plan(w.read, W, None, True, BITS, 'auto')
    assert (admitted, filter_bytes, P, slots, budget) == (ADMITTED, 16 * WORDS, 3, 65536, M2) and filt is w.filters[0] and filt.closed == 0
    assert w.log == [('filter', WORDS), 'prefilter', 'release_seen']
    del w.log[:]
    hist, kept, info = kmer.count_rounds(lambda table, p: w.read('count', table=table, parts=1, part=p), 21, 1, 2048, 1)
    assert w.log == [('table', 2048), ('count', 1, 0), 'hist', 'select', 'table.close']
    assert info == dict(partitions=1, slots=2048, table_bytes=24576) and int(hist[1]) == 6 and len(kept) == 1 and kept[0][0].size == 17
    del w.log[:]
    hist, kept, info = kmer.count_rounds(lambda table, p: w.read('count', table=table, parts=2, part=p), 21, 2, 2048, 4)
    assert w.log == [('table', 2048), ('count', 2, 0), 'hist', 'select', 'clear', ('count', 2, 1), 'hist', 'select', 'table.close']
    assert int(hist.sum()) == 17 and sum(k.size for k, _ in kept) == 7 and info['partitions'] == 2
