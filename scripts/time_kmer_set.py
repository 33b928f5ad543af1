#!/usr/bin/env python3
"""Timing of the k-mer set path beside the count it replaces, on device-resident synthetic reads (the generator of
scripts/time_correct.py: `--reads` x `--len` bases from both strands of a random genome at `--depth` x, `--err` substitutions).
Device steps are timed with HIP events, median of `--reps` after one warm-up: the count into a fresh table, the histogram, the
select of the pairs with count >= `--keep`, the sort (kbbq_kmer_sort_pairs_dev), the check (kbbq_kmer_check_pairs_dev, which
synchronises: its figure includes one small download) and the correct step.  The steps with a file in them are wall clock,
median of `--reps`: the download and write of the set, and kmer.load_set (read, upload, check, merge) of it.  Prints one JSON
line: ms per step, pairs per second of the sort and the check, the set's pairs and bytes, and the two sums the issue asks for:
count_ms = count + histogram (what every k-mer command pays today before it decides) and load_ms (what --kmers-from pays)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=4_000_000)
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--depth', type=float, default=30.0)
ap.add_argument('--err', type=float, default=0.01)
ap.add_argument('-k', type=int, default=31)
ap.add_argument('--keep', type=int, default=2)
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()

import numpy as np
import torch
from kbbq import _device as dev
from kbbq import kmer, kmerset

n, L, k = args.reads, args.len, args.k
pitch = (L + 15) // 16 * 16
G = max(int(n * L / args.depth), 10 * L)
g = torch.Generator(device='cuda').manual_seed(5)
genome = torch.randint(0, 4, (G,), device='cuda', generator=g, dtype=torch.uint8)
seq = torch.full((n, pitch), ord('N'), dtype=torch.uint8, device='cuda')
acgt = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device='cuda')
col = torch.arange(L, device='cuda')
step = 1 << 22
for lo in range(0, n, step):
    m = min(step, n - lo)
    start = torch.randint(0, G - L + 1, (m, 1), device='cuda', generator=g)
    b = genome[start + col]
    b = torch.where(torch.rand((m, 1), device='cuda', generator=g) < 0.5, (3 - b).flip(1), b)
    err = torch.rand((m, L), device='cuda', generator=g) < args.err
    b = torch.where(err, (b + torch.randint(1, 4, (m, L), device='cuda', generator=g, dtype=torch.uint8)) % 4, b)
    seq[lo:lo + m, :L] = acgt[b.long()]
del genome
meta = torch.full((n,), L, dtype=torch.int32, device='cuda')
windows = n * max(L - k + 1, 0)
slots = 1 << int(np.ceil(np.log2((G + windows * args.err * k) * 2)))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


ms = {name: [] for name in ('count', 'histogram', 'select', 'sort', 'check', 'write', 'load', 'correct', 'correct_loaded')}
tmp = tempfile.mkdtemp()
facts = {}
for rep in range(args.reps + 1):
    keepit = rep > 0                                       # repetition 0 warms up
    table = kmer.KmerTable(k, slots)
    t_count, _ = timed(lambda: kmer.count_kmers(seq, meta, table=table))
    t_hist, hist = timed(lambda: kmer.kmer_histogram(table))
    t = kmer.solid_threshold(hist)
    t_correct, (plain, _) = timed(lambda: kmer.correct_with(table, seq, meta, t))
    t_select, (keys, counts, _) = timed(lambda: kmer.select(table, 1, args.keep))
    table.close()
    pairs = int(keys.shape[0])
    t_sort, (skeys, scounts) = timed(lambda: kmer.sort_pairs([(keys, counts)], k))
    del keys, counts
    t_check, (sums, bad) = timed(lambda: kmer.check_pairs(skeys, scounts, k, args.keep))
    assert bad is None
    h = hist.copy()
    h[:args.keep] = 0
    path = os.path.join(tmp, 'rep%d.kset' % rep)
    slab = kmerset.slab_pairs()
    T = dev._torch()
    t_write, _ = wall(lambda: kmerset.write_set(
        path, k, args.keep, 0, n, windows, h, int(sums[0]), int(sums[1]),
        lambda what: kmerset._download(T, dev, skeys if what == 'keys' else scounts, pairs, np.uint64 if what == 'keys' else np.uint32, slab),
        pairs))
    del skeys, scounts
    t_load, (loaded, _, t2, info) = wall(lambda: kmer.load_set(path))
    assert t2 == t and info['loaded_kmers'] == pairs
    t_correct2, (again, _) = timed(lambda: kmer.correct_with(loaded, seq, meta, t))
    same = bool(torch.equal(plain, again))
    loaded.close()
    facts = dict(pairs=pairs, set_bytes=os.path.getsize(path), min_count=t, same_plane=same, table_bytes=slots * 12,
                 loaded_table_bytes=info['table_bytes'])
    os.unlink(path)
    del plain, again
    if keepit:
        for name, v in (('count', t_count), ('histogram', t_hist), ('select', t_select), ('sort', t_sort), ('check', t_check),
                        ('write', t_write), ('load', t_load), ('correct', t_correct), ('correct_loaded', t_correct2)):
            ms[name].append(v)
med = {name: statistics.median(v) for name, v in ms.items()}
print(json.dumps(dict(reads=n, len=L, k=k, keep=args.keep, windows=windows, **facts,
                      ms={name: round(v, 3) for name, v in med.items()},
                      count_ms=round(med['count'] + med['histogram'], 3), load_ms=round(med['load'], 3),
                      sort_pairs_per_s=round(facts['pairs'] / (med['sort'] * 1e-3)), check_pairs_per_s=round(facts['pairs'] / (med['check'] * 1e-3)),
                      device=dev.context().name)))
