#!/usr/bin/env python3
"""Kernel timing (HIP events) of ApplyBQSR on aligned rows (kbbq_apply_aligned_dev) on device-resident synthetic character planes:
16 M alignments x 150 bases by default, both strands, first and second of pair, 2 read groups, the integer-LUT and the exact
float64 form of the model.  Prints one JSON line per form: ms per launch, G bases/s and the fraction of 8 TB/s on algorithmic
bytes (SEQ + source + output = 3 B/base with the context taken from the source plane; 4 B/base with a separate OQ plane)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=16_000_000)
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--rgs', type=int, default=2)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--separate-oq', action='store_true', help='source QUAL, context from a separate OQ plane (4 B/base)')
args = ap.parse_args()

import numpy as np
import torch
from kbbq import _device as dev
from kbbq import _native as N
from kbbq.gatk import applybqsr

n, L, R = args.reads, args.len, args.rgs
pitch = (L + 15) // 16 * 16
g = torch.Generator(device='cuda').manual_seed(3)
acgt = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device='cuda')
col = torch.arange(pitch, device='cuda') < L
seq = torch.where(col, acgt[torch.randint(0, 4, (n, pitch), device='cuda', generator=g)], torch.zeros((), dtype=torch.uint8, device='cuda'))
qual = torch.where(col, torch.randint(33 + 2, 33 + 42, (n, pitch), device='cuda', generator=g, dtype=torch.uint8),
                   torch.zeros((), dtype=torch.uint8, device='cuda'))
oq = torch.where(col, torch.randint(33 + 2, 33 + 42, (n, pitch), device='cuda', generator=g, dtype=torch.uint8),
                 torch.zeros((), dtype=torch.uint8, device='cuda')) if args.separate_oq else qual
flags = torch.randint(0, 4, (n,), device='cuda', generator=g, dtype=torch.int64)
rg = torch.randint(0, R, (n,), device='cuda', generator=g, dtype=torch.int64)
src_oq = 0 if args.separate_oq else 1 << 28
meta = L | (rg << 16) | src_oq | (1 << 29) | ((flags & 1) << 30) | ((flags >> 1) << 31)
meta = ((meta + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)          # the uint32 row words, as int32
out = torch.empty_like(seq)
ctx = dev.context()
rng = np.random.default_rng(5)
ints = [rng.integers(20, 35, R), rng.integers(-2, 3, R), rng.integers(-4, 5, (R, 43)), rng.integers(-3, 4, (R, 43, 2 * L)),
        np.concatenate([rng.integers(-3, 4, (R, 43, 16)), np.zeros((R, 43, 1), np.int64)], -1)]
flts = [x + rng.uniform(-0.5, 0.5, np.shape(x)) for x in ints]
flts[4][..., 16] = 0.0
lib = N.load()
bytes_per_base = 4 if args.separate_oq else 3
for name, model in (('lut', ints), ('f64', flts)):
    mode, blob, R_, Qt, S2 = applybqsr._model(*model, 6)
    assert (mode == N.ALIGNED_LUT) == (name == 'lut'), (name, mode)
    d_model = torch.from_numpy(blob).cuda()

    def run():
        N.check(lib.kbbq_apply_aligned_dev(ctx.handle, N.ptr(seq), N.ptr(qual), N.ptr(oq), N.ptr(meta), n, pitch, R_, Qt, S2, 6,
                                           N.ptr(d_model), mode, N.ptr(out)))
    run()
    ctx.status()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ctx.status()
    best, med = min(ms), sorted(ms)[len(ms) // 2]
    bases = n * L
    print(json.dumps(dict(form=name, reads=n, length=L, read_groups=R, bytes_per_base=bytes_per_base, ms_best=round(best, 3),
                          ms_median=round(med, 3), gbases_per_s=round(bases / best / 1e6, 1),
                          fraction_of_8tbs=round(bases * bytes_per_base / (best * 1e-3) / 8e12, 3))), flush=True)
