"""kbbq correct across ranks, the parts that need no GPU: the owner rule (kmer.owner against a restatement written here and
against the library's kbbq_kmer_owner), the balance of the owners and their independence from the home slot, and the
collectives of kbbq/parallel.py (all_to_all_rows, all_gather_rows, sum_over_ranks) on 4 gloo CPU ranks."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

M64 = (1 << 64) - 1


def _mix_int(x):
    """km_hash on one Python int."""
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def _owner_int(key, world):
    return ((_mix_int(key ^ 0x9E3779B97F4A7C15) >> 32) * world) >> 32


def _canonical_keys(n, k, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 1 << (2 * k), size=n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        rc = (rc << np.uint64(2)) | (np.uint64(3) - ((f >> np.uint64(2 * i)) & np.uint64(3)))
    return np.minimum(f, rc)


def test_owner_equals_a_restatement_and_the_library():
    from kbbq import _native as N
    from kbbq import kmer
    keys = np.concatenate([_canonical_keys(2000, 31, 1), _canonical_keys(500, 8, 2),
                           np.array([0, 1, (1 << 62) - 1, (1 << 64) - 2], dtype=np.uint64)])
    lib = N.load()
    for world in (1, 2, 3, 7, 8, 1000, 1024):
        got = kmer.owner(keys, world)
        assert got.dtype == np.uint32 and got.shape == keys.shape
        want = np.array([_owner_int(int(x), world) for x in keys], dtype=np.uint32)
        assert np.array_equal(got, want), world
        assert int(got.max()) < world
        assert all(int(lib.kbbq_kmer_owner(int(x), world)) == int(o) for x, o in zip(keys[:300], got[:300]))


def test_owners_share_the_keys_evenly():
    from kbbq import kmer
    keys = _canonical_keys(1_000_000, 31, 3)
    share = np.bincount(kmer.owner(keys, 8), minlength=8) / keys.size
    assert np.all(np.abs(share - 1 / 8) < 0.01 / 8), share


def test_owned_keys_spread_over_every_home_slot():
    """The keys one rank owns must not crowd into part of its table: their home slots (km_hash(key) & mask) are spread as
    evenly as all keys' are, in the low bits (neighbouring slots) and in the high ones (regions of the table)."""
    from kbbq import kmer
    keys = _canonical_keys(1_000_000, 31, 4)
    own = kmer.owner(keys, 8)
    with np.errstate(over='ignore'):
        home = kmer._mix(keys) & np.uint64((1 << 20) - 1)
    for r in (0, 5):
        mine = home[own == r]
        low = np.bincount((mine & np.uint64(7)).astype(np.int64), minlength=8) / mine.size
        high = np.bincount((mine >> np.uint64(14)).astype(np.int64), minlength=64) / mine.size
        assert np.all(np.abs(low - 1 / 8) < 0.05 / 8), low
        assert np.all(np.abs(high - 1 / 64) < 0.15 / 64), high


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _rows_of(src, dst, n):
    """Rows rank `src` sends to rank `dst`: n rows of (src, dst, i, src * 1000 + dst * 10 + i)."""
    return [[src, dst, i, src * 1000 + dst * 10 + i] for i in range(n)]


def _send_count(src, dst):
    return (src * 3 + dst * 5) % 4 if src != 2 else 0            # uneven; rank 2 sends nothing; some pairs get nothing


def _collectives_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from kbbq import parallel
        ok = all(_exchanges(parallel, rank, world, limit) for limit in (parallel.EXCHANGE_BYTES, 40))
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


def _exchanges(parallel, rank, world, limit):
    """The collectives with calls of at most `limit` bytes per rank (40: one row of four int64 per destination and call)."""
    parallel.EXCHANGE_BYTES = limit
    sizes = [_send_count(rank, d) for d in range(world)]
    rows = sum((_rows_of(rank, d, sizes[d]) for d in range(world)), [])
    send = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    got, recv = parallel.all_to_all_rows(send, sizes)
    want = sum((_rows_of(s, rank, _send_count(s, rank)) for s in range(world)), [])
    ok = got.tolist() == want and recv == [_send_count(s, rank) for s in range(world)]
    # a second payload with the sizes already known (1-d, int32)
    got1, recv1 = parallel.all_to_all_rows(send[:, 3].to(torch.int32), sizes, recv)
    ok = ok and got1.tolist() == [w[3] for w in want] and recv1 == recv
    # gather: rank 1 has no rows, the others 2 * rank + 1
    n = 0 if rank == 1 else 2 * rank + 1
    mine = torch.arange(n, dtype=torch.int64) + 100 * rank
    gathered = parallel.all_gather_rows(mine)
    ok = ok and gathered.tolist() == sum(([100 * r + i for i in range(0 if r == 1 else 2 * r + 1)] for r in range(world)), [])
    total = parallel.sum_over_ranks(np.array([rank, 1, 1 << 40], dtype=np.int64))
    ok = ok and total.tolist() == [sum(range(world)), world, world << 40]
    return ok


def test_rank_collectives_on_four_gloo_ranks():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    world = 4
    procs = [ctx.Process(target=_collectives_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == {r: True for r in range(world)}


def test_collectives_without_a_process_group():
    from kbbq import parallel
    t = torch.arange(6)
    got, sizes = parallel.all_to_all_rows(t, [6])
    assert got.tolist() == list(range(6)) and sizes == [6]
    assert parallel.all_gather_rows(t) is t
    assert parallel.sum_over_ranks([3, 4]).tolist() == [3, 4]


def test_rounds_cover_the_rows_in_order():
    from kbbq import kmer
    lens = np.array([150, 0, 40, 300, 31, 30, 150, 150, 1000 - 1], dtype=np.uint32)
    w = np.maximum(lens.astype(np.int64) - 31 + 1, 0)
    for cap in (1, 100, 200, 500, 10_000):
        rounds = kmer._rounds(lens, 31, cap)
        assert rounds[0][0] == 0 and rounds[-1][1] == lens.size
        assert all(a[1] == b[0] for a, b in zip(rounds, rounds[1:]))
        assert all(w[lo:hi].sum() <= cap or hi - lo == 1 for lo, hi in rounds)
    assert kmer._rounds(lens[:0], 31, 10) == []
