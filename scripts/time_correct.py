#!/usr/bin/env python3
"""Kernel timing (HIP events) of kbbq correct's three steps on device-resident synthetic reads: `--reads` x `--len` bases
sampled from both strands of a random genome sized for `--depth` x coverage, `--err` uniform substitutions.  Count
(kbbq_kmer_count_dev into a fresh table), histogram (kbbq_kmer_histogram_dev) and correct (kbbq_kmer_correct_dev) are each
timed once per repetition after a warm-up on the same table.  Prints one JSON line: ms per step, k-mer windows per second of
the count and of the correct step, the table's slots and bytes, its distinct k-mers, the threshold and the changed bases."""
import argparse
import ctypes
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
ap.add_argument('--slots', type=int, default=0, help='table slots (default: distinct k-mers expected at a load factor <= 0.5)')
ap.add_argument('--reps', type=int, default=3)
args = ap.parse_args()

import numpy as np
import torch
from kbbq import _native as N
from kbbq import kmer

n, L, k = args.reads, args.len, args.k
pitch = (L + 15) // 16 * 16
G = max(int(n * L / args.depth), 10 * L)
g = torch.Generator(device='cuda').manual_seed(5)
genome = torch.randint(0, 4, (G,), device='cuda', generator=g, dtype=torch.uint8)
seq = torch.full((n, pitch), ord('N'), dtype=torch.uint8, device='cuda')
acgt = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device='cuda')
col = torch.arange(L, device='cuda')
step = 1 << 22
for lo in range(0, n, step):                         # slices: the index tensors of all reads at once would not fit beside the planes
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
distinct = G + windows * args.err * k                  # the genome's k-mers and those an error makes
slots = args.slots or 1 << int(np.ceil(np.log2(distinct * 2)))
out = torch.empty_like(seq)
lib = N.load()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


res = {'reads': n, 'len': L, 'k': k, 'genome': G, 'err': args.err, 'slots': slots,
       'table_bytes': int(lib.kbbq_kmer_table_bytes(slots))}
ms = {'count': [], 'histogram': [], 'correct': []}
dh = torch.zeros(257, dtype=torch.int64, device='cuda')
for rep in range(args.reps + 1):
    table = kmer.KmerTable(k, slots)
    torch.cuda.synchronize()
    c = timed(lambda: N.check(lib.kbbq_kmer_count_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch)))
    table.ctx.status()
    h = timed(lambda: N.check(lib.kbbq_kmer_histogram_dev(table.ctx.handle, table.handle, N.ptr(dh))))
    hist = dh.cpu().numpy()
    t = kmer.solid_threshold(hist)
    x = timed(lambda: N.check(lib.kbbq_kmer_correct_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                         N.ptr(out), None)))
    table.close()
    if rep:                                            # the first round is the warm-up
        ms['count'].append(c); ms['histogram'].append(h); ms['correct'].append(x)
res.update({'ms_' + key: round(float(np.median(v)), 3) for key, v in ms.items()})
res['count_kmers_per_s'] = windows / (res['ms_count'] * 1e-3)
res['correct_kmers_per_s'] = windows / (res['ms_correct'] * 1e-3)
res['distinct'] = int(hist.sum())
res['load_factor'] = round(res['distinct'] / slots, 3)
res['min_count'] = t
res['changed_bases'] = int((out != seq).sum().item())
print(json.dumps(res))
