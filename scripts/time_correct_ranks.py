#!/usr/bin/env python3
"""Timing (HIP events) of `kbbq correct`'s rank path against the one-process path on device-resident synthetic reads, the
reads of scripts/time_correct.py (`--reads` x `--len` bases from both strands of a random genome at `--depth` x, `--err`
uniform substitutions).  Run it as a rank of a process group, e.g. one MI355X as a one-rank RCCL group:

    KBBQ_DIST_ALWAYS=1 python -m torch.distributed.run --nproc-per-node 1 scripts/time_correct_ranks.py

One process: count (kbbq_kmer_count_dev), histogram, correct against the counted table.  Rank path: count into the local
table, km_select_sizes and km_select_scatter into one bucket per rank, the exchange (all_to_all_rows of keys and counts),
km_merge into the owner table, histogram and its sum over ranks, the solid select (one bucket, min_count = t), the gather
of the solid set, the solid table's build (create + km_merge) and correct against it.  `--buckets` also times a select
into that many buckets (the partition of a node of that many GPUs).  Both tables have `--slots` slots (default: the
expected distinct k-mers at a load factor <= 0.5).  Median of `--reps` repetitions after a warm-up; one JSON line from rank 0."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=16_000_000)
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--depth', type=float, default=30.0)
ap.add_argument('--err', type=float, default=0.01)
ap.add_argument('-k', type=int, default=31)
ap.add_argument('--slots', type=int, default=0)
ap.add_argument('--buckets', type=int, default=8)
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()

import numpy as np
import torch
from kbbq import _native as N
from kbbq import kmer, parallel

world, rank = parallel.init_from_env()
n, L, k = args.reads, args.len, args.k
pitch = (L + 15) // 16 * 16
G = max(int(n * L / args.depth), 10 * L)
g = torch.Generator(device='cuda').manual_seed(5 + rank)
genome = torch.randint(0, 4, (G,), device='cuda', generator=torch.Generator(device='cuda').manual_seed(5), dtype=torch.uint8)
seq = torch.full((n, pitch), ord('N'), dtype=torch.uint8, device='cuda')
acgt = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device='cuda')
col = torch.arange(L, device='cuda')
step = 1 << 22
for lo in range(0, n, step):
    m = min(step, n - lo)
    start = torch.randint(0, G - L + 1, (m, 1), device='cuda', generator=g)
    b = genome[start + col]
    rev = torch.rand((m, 1), device='cuda', generator=g) < 0.5
    b = torch.where(rev, (3 - b).flip(1), b)
    err = torch.rand((m, L), device='cuda', generator=g) < args.err
    b = torch.where(err, (b + torch.randint(1, 4, (m, L), device='cuda', generator=g, dtype=torch.uint8)) % 4, b)
    seq[lo:lo + m, :L] = acgt[b.long()]
del genome
meta = torch.full((n,), L, dtype=torch.int32, device='cuda')
windows = n * max(L - k + 1, 0)
distinct = G + windows * args.err * k
slots = args.slots or 1 << int(np.ceil(np.log2(distinct * 2)))
out = torch.empty_like(seq)
lib = N.load()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def count(table):
    N.check(lib.kbbq_kmer_count_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch))
    table.ctx.status()


def correct(table, t):
    N.check(lib.kbbq_kmer_correct_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t, N.ptr(out), None))


def sizes_only(table, nb):
    s = np.zeros(nb, dtype=np.int64)
    N.check(lib.kbbq_kmer_select_sizes_dev(table.ctx.handle, table.handle, nb, 1, N.ptr(s)))
    return s


def exchange(keys, counts, sizes):
    rk, got = parallel.all_to_all_rows(keys, sizes)
    rc, _ = parallel.all_to_all_rows(counts, sizes, got)
    return rk, rc


def one_process():
    ms = {}
    table = kmer.KmerTable(k, slots)
    ms['count'], _ = timed(lambda: count(table))
    ms['histogram'], hist = timed(lambda: kmer.kmer_histogram(table))
    t = kmer.solid_threshold(hist)
    ms['correct'], _ = timed(lambda: correct(table, t))
    table.close()
    ms['total'] = sum(ms.values())
    return ms, t, hist


def rank_path():
    ms = {}
    local = kmer.KmerTable(k, slots)
    ms['count'], _ = timed(lambda: count(local))
    ms['select_sizes'], _ = timed(lambda: sizes_only(local, world))
    ms['select'], (keys, counts, sizes) = timed(lambda: kmer.select(local, world, 1))       # sizes and scatter
    ms['select_scatter'] = ms['select'] - ms['select_sizes']
    ms['select_sizes_%d' % args.buckets], _ = timed(lambda: sizes_only(local, args.buckets))
    ms['select_%d' % args.buckets], sel = timed(lambda: kmer.select(local, args.buckets, 1))
    del sel
    local.close()
    ms['exchange'], (rk, rc) = timed(lambda: exchange(keys, counts, sizes))
    intact = world > 1 or (bool(torch.equal(rk, keys)) and bool(torch.equal(rc, counts)))
    del keys, counts
    owned = kmer.KmerTable(k, slots)
    ms['merge'], _ = timed(lambda: kmer.merge(owned, rk, rc))
    merged = int(rk.shape[0])
    del rk, rc
    ms['histogram'], hist = timed(lambda: kmer.kmer_histogram_ranks(owned))
    t = kmer.solid_threshold(hist)
    ms['solid_select'], (sk, sc, _) = timed(lambda: kmer.select(owned, 1, t))
    owned.close()
    ms['gather'], (gk, gc) = timed(lambda: (parallel.all_gather_rows(sk), parallel.all_gather_rows(sc)))
    nsolid = int(gk.shape[0])
    ms['solid_build'], solid = timed(lambda: kmer.merge(kmer.KmerTable(k, kmer.default_slots(nsolid, 1 << 42)), gk, gc))
    del sk, sc, gk, gc
    ms['correct'], _ = timed(lambda: correct(solid, t))
    solid_slots = solid.slots
    solid.close()
    ms['total'] = sum(v for key, v in ms.items() if key in ('count', 'select', 'exchange', 'merge', 'histogram', 'solid_select',
                                                             'gather', 'solid_build', 'correct'))
    return ms, t, merged, nsolid, solid_slots, hist, intact


runs1, runsr = [], []
for rep in range(args.reps + 1):
    a = one_process()
    b = rank_path()
    if rep:
        runs1.append(a[0]); runsr.append(b[0])
    changed = int((out != seq).sum().item())
med = lambda runs: {key: round(float(np.median([r[key] for r in runs])), 3) for key in runs[0]}
res = {'reads': n, 'len': L, 'k': k, 'world': world, 'backend': torch.distributed.get_backend() if torch.distributed.is_initialized() else None,
       'slots': slots, 'table_bytes': int(lib.kbbq_kmer_table_bytes(slots)), 'min_count': a[1], 'rank_min_count': b[1],
       'histogram_equal': bool(np.array_equal(a[2], b[5])), 'exchange_intact': b[6], 'pairs_merged': b[2], 'solid': b[3], 'solid_slots': b[4], 'changed_bases_rank_path': changed,
       'ms_one_process': med(runs1), 'ms_rank_path': med(runsr)}
r = res['ms_rank_path']
res['merge_pairs_per_s'] = b[2] / (r['merge'] * 1e-3)
res['select_slots_per_s'] = slots / (r['select'] * 1e-3)
res['rank_over_one'] = round(r['total'] / res['ms_one_process']['total'], 3)
if rank == 0:
    print(json.dumps(res))
