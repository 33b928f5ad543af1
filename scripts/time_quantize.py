#!/usr/bin/env python3
"""Kernel timing (HIP events) of static quantized qualities (--static-quantized-quals):
  plane    kbbq_quantize_plane_dev on the resident quality plane K2 has just written for the headline shape (bench.py: 50 M
           synthetic 2x150 reads, 1 read group, the packed layout -- mate-pair rows), next to K2's own time in the same process;
           ms, G bases/s and the fraction of 8 TB/s on 2 B/base (1 read + 1 written)
  aligned  kbbq_apply_aligned_q_dev against kbbq_apply_aligned_dev on scripts/time_applybqsr.py's planes (16 M alignments x 150
           bases, 2 read groups; the integer-LUT and the float64 form), the two calls alternating
One JSON line each.  usage (GPU box): python scripts/time_quantize.py [--reads N] [--aligned-reads N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=50_000_000, help='reads of the headline shape (plane pass)')
ap.add_argument('--aligned-reads', type=int, default=16_000_000, help='alignments of the aligned apply')
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--levels', default='10,20,30,40')
args = ap.parse_args()

import numpy as np
import torch
from kbbq import _device as dev
from kbbq import _native as N
from kbbq.gatk import applybqsr

ctx, lib = dev.context(), N.load()
table = applybqsr.quantize_map([int(x) for x in args.levels.split(',')])
qmap = dev.qmap_to_device(table)


def timed(fn, reps):
    fn()
    ctx.status()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ctx.status()
    return min(ms), sorted(ms)[len(ms) // 2]


# ---- the plane pass behind K2, headline shape
n, S, R = args.reads, args.len, 1
batch = dev.ReadBatch.synthetic(0, n, n, seed=1, nrg=R)
tables = dev.Tables(R, 2 * S)
dev.accumulate(batch, tables)
lut, shape = dev.solve_lut(tables)
laid = dev.lay_out(batch, R, S, packed=True)
del batch
out = torch.empty_like(laid.qual)
k2 = timed(lambda: dev.apply(laid, lut, shape, out=out, check=False), args.reps)
keep = out.clone()
nbytes = int(out.numel())


def plane():
    N.check(lib.kbbq_quantize_plane_dev(ctx.handle, N.ptr(out), nbytes, N.ptr(qmap)))
q = timed(plane, args.reps)
sample = slice(0, min(1 << 16, out.shape[0]))
same = bool(np.array_equal(out[sample].cpu().numpy(), table[keep[sample].cpu().numpy()]))
bases = n * S
print(json.dumps(dict(what='plane', reads=n, length=S, layout=laid.describe(), plane_bytes=nbytes, verified=same,
                      k2_ms_best=round(k2[0], 3), k2_ms_median=round(k2[1], 3),
                      quantize_ms_best=round(q[0], 3), quantize_ms_median=round(q[1], 3),
                      quantize_gbases_per_s=round(bases / q[0] / 1e6, 1),
                      quantize_fraction_of_8tbs_on_plane_bytes=round(2 * nbytes / (q[0] * 1e-3) / 8e12, 3),
                      quantize_fraction_of_8tbs_on_2B_per_base=round(2 * bases / (q[0] * 1e-3) / 8e12, 3),
                      quantize_over_k2=round(q[0] / k2[0], 3))), flush=True)
del laid, out, keep, tables, lut

# ---- the fused aligned apply against the plain one, time_applybqsr.py's planes
n, L, R = args.aligned_reads, args.len, 2
pitch = (L + 15) // 16 * 16
g = torch.Generator(device='cuda').manual_seed(3)
acgt = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device='cuda')
col = torch.arange(pitch, device='cuda') < L
zero = torch.zeros((), dtype=torch.uint8, device='cuda')
seq = torch.where(col, acgt[torch.randint(0, 4, (n, pitch), device='cuda', generator=g)], zero)
qual = torch.where(col, torch.randint(33 + 2, 33 + 42, (n, pitch), device='cuda', generator=g, dtype=torch.uint8), zero)
flags = torch.randint(0, 4, (n,), device='cuda', generator=g, dtype=torch.int64)
rg = torch.randint(0, R, (n,), device='cuda', generator=g, dtype=torch.int64)
meta = L | (rg << 16) | (1 << 28) | (1 << 29) | ((flags & 1) << 30) | ((flags >> 1) << 31)
meta = ((meta + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)          # the uint32 row words, as int32
out = torch.empty_like(seq)
rng = np.random.default_rng(5)
ints = [rng.integers(20, 35, R), rng.integers(-2, 3, R), rng.integers(-4, 5, (R, 43)), rng.integers(-3, 4, (R, 43, 2 * L)),
        np.concatenate([rng.integers(-3, 4, (R, 43, 16)), np.zeros((R, 43, 1), np.int64)], -1)]
flts = [x + rng.uniform(-0.5, 0.5, np.shape(x)) for x in ints]
flts[4][..., 16] = 0.0
for name, model in (('lut', ints), ('f64', flts)):
    mode, blob, R_, Qt, S2 = applybqsr._model(*model, 6)
    d_model = torch.from_numpy(blob).cuda()
    common = (ctx.handle, N.ptr(seq), N.ptr(qual), N.ptr(qual), N.ptr(meta), n, pitch, R_, Qt, S2, 6, N.ptr(d_model), mode, N.ptr(out))
    plain_ms, q_ms = [], []
    for fn in (lambda: N.check(lib.kbbq_apply_aligned_dev(*common)), lambda: N.check(lib.kbbq_apply_aligned_q_dev(*common, N.ptr(qmap)))):
        fn()                                                                  # first launches: code load
    ctx.status()
    torch.cuda.synchronize()
    for _ in range(args.reps):                                                # alternating, so that drift falls on both
        for ms, fn in ((plain_ms, lambda: N.check(lib.kbbq_apply_aligned_dev(*common))),
                       (q_ms, lambda: N.check(lib.kbbq_apply_aligned_q_dev(*common, N.ptr(qmap))))):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    ctx.status()
    bases = n * L
    print(json.dumps(dict(what='aligned', form=name, reads=n, length=L, read_groups=R, bytes_per_base=3,
                          plain_ms_best=round(min(plain_ms), 3), plain_ms_median=round(sorted(plain_ms)[len(plain_ms) // 2], 3),
                          plain_ms_spread=round(max(plain_ms) - min(plain_ms), 3),
                          q_ms_best=round(min(q_ms), 3), q_ms_median=round(sorted(q_ms)[len(q_ms) // 2], 3),
                          q_ms_spread=round(max(q_ms) - min(q_ms), 3),
                          q_over_plain_median=round(sorted(q_ms)[len(q_ms) // 2] / sorted(plain_ms)[len(plain_ms) // 2], 4),
                          q_fraction_of_8tbs=round(bases * 3 / (min(q_ms) * 1e-3) / 8e12, 3))), flush=True)
