#!/usr/bin/env python3
"""Measurements of --bgzf on one GPU, on the output of `kbbq recalibrate -f A B` for `--reads` synthetic 150-base reads (8 M by
default: 2.5 GB of FASTQ text; the files are written under TMPDIR and removed).
  kernel     kbbq_bgzf_deflate_dev on device-resident slabs of that text (`--slab-blocks` blocks of 65280 bytes each), HIP events
             around the call, per slab the median of `--reps` after one warm-up; GB/s of text over the sum of the medians.
  sizes      the packed length against zlib level 1, level 6 and Z_HUFFMAN_ONLY (raw deflate + the 26 bytes of a BGZF block) on
             the same 65280-byte cuts, every block of the file, `--threads` host threads.
  wall       the command line as a process, wall clock, median of `--reps` after one warm-up, a fresh output file each time:
             plain -o, --bgzf -o, and plain stdout piped through `gzip -1`.
Prints progress lines and one JSON line at the end.  usage (GPU box): python scripts/time_bgzf.py [--reads N]"""
import argparse
import concurrent.futures
import ctypes
import gzip
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=8_000_000)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--slab-blocks', type=int, default=4096)
ap.add_argument('--threads', type=int, default=16)
ap.add_argument('--no-gzip', action='store_true', help='skip the `| gzip -1` runs (half a minute each at 8 M reads)')
args = ap.parse_args()

import numpy as np
import torch
from kbbq import _device as dev
from kbbq import _native as N

BLOCK = N.BGZF_BLOCK_MAX
n = args.reads
tmp = os.environ.get('TMPDIR', '/tmp')
fa, fb, fo, fz = (os.path.join(tmp, 'kbbq_bgzf_%d_%s' % (os.getpid(), x)) for x in ('a.fq', 'b.fq', 'out.fq', 'out.fq.gz'))


def say(*what):
    print(*what, flush=True)


def write_inputs():
    batch = dev.ReadBatch.synthetic(0, n, n, seed=1)
    seq, cseq, qual = (getattr(batch, p).cpu().numpy()[:n, :150] for p in ('seq', 'cseq', 'qual'))
    del batch
    for path, plane in ((fa, seq), (fb, cseq)):
        rec = np.empty((n, 318), dtype=np.uint8)
        ids = np.arange(n)
        rec[:, 0] = ord('@'); rec[:, 1] = ord('r'); rec[:, 11] = ord('/')
        rec[:, 2:11] = ((ids >> 1)[:, None] // 10 ** np.arange(8, -1, -1)[None, :] % 10 + 48).astype(np.uint8)
        rec[:, 12] = 49 + (ids & 1); rec[:, 13] = 10
        rec[:, 14:164] = plane; rec[:, 164] = 10; rec[:, 165] = ord('+'); rec[:, 166] = 10
        rec[:, 167:317] = qual; rec[:, 317] = 10
        rec.tofile(path)
        del rec


ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH'):
    ENV.pop(var, None)
KBBQ = '%s -m kbbq.main recalibrate -f %s %s' % (sys.executable, fa, fb)


def wall(label, command, out):
    times = []
    for rep in range(args.reps + 1):
        if os.path.exists(out):
            os.remove(out)                   # a fresh output file: truncating gigabytes of page cache is not the command's time
        t0 = time.perf_counter()
        subprocess.run(command, shell=True, check=True, env=ENV)       # no timeout: with one the wait polls every 0.05 s
        times.append(time.perf_counter() - t0)
        say('  %s: repetition %d %.3f s, %d bytes' % (label, rep, times[-1], os.path.getsize(out)))
    return statistics.median(times[1:]), os.path.getsize(out)


def zlib_sizes(text):
    """Bytes of the BGZF blocks zlib would make of the 65280-byte cuts of `text`, for the three settings."""
    def one(lo):
        piece = text[lo:lo + BLOCK]
        out = []
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY)):
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            out.append(len(c.compress(piece)) + len(c.flush()) + 26)
        return out
    with concurrent.futures.ThreadPoolExecutor(args.threads) as pool:
        sums = np.array(list(pool.map(one, range(0, len(text), BLOCK))), dtype=np.int64).sum(axis=0)
    return dict(zlib_1=int(sums[0]), zlib_6=int(sums[1]), zlib_huffman_only=int(sums[2]))


try:
    say('writing %d reads ...' % n)
    write_inputs()
    result = dict(reads=n, device=dev.context().name, reps=args.reps)
    say('wall: plain -o')
    result['wall_plain_s'], result['text_bytes'] = wall('plain', '%s -o %s' % (KBBQ, fo), fo)
    text = np.fromfile(fo, dtype=np.uint8)
    say('wall: --bgzf -o')
    result['wall_bgzf_s'], result['bgzf_bytes'] = wall('--bgzf', '%s --bgzf -o %s' % (KBBQ, fz), fz)
    with gzip.open(fz, 'rb') as fh:                                   # the file is the text
        at = 0
        while True:
            piece = fh.read(1 << 26)
            if not piece:
                break
            assert piece == text[at:at + len(piece)].tobytes(), 'the --bgzf output does not inflate to the plain output'
            at += len(piece)
        assert at == text.size
    if not args.no_gzip:
        say('wall: plain | gzip -1')
        result['wall_gzip1_pipe_s'], result['gzip1_pipe_bytes'] = wall('| gzip -1', '%s | gzip -1 > %s' % (KBBQ, fz), fz)
    say('kernel: slabs of %d blocks' % args.slab_blocks)
    lib, ctx = N.load(), dev.context()
    slab = args.slab_blocks * BLOCK
    bound = int(lib.kbbq_bgzf_bound(slab, BLOCK))
    d_text = torch.empty(slab, dtype=torch.uint8, device='cuda')
    d_blocks = torch.empty(args.slab_blocks * N.BGZF_SLOT, dtype=torch.uint8, device='cuda')
    d_sizes = torch.empty(args.slab_blocks, dtype=torch.int32, device='cuda')
    d_packed = torch.empty(bound, dtype=torch.uint8, device='cuda')
    total, ms, packed = ctypes.c_size_t(0), 0.0, 0
    for lo in range(0, text.size, slab):
        m = min(slab, text.size - lo)
        d_text[:m].copy_(torch.from_numpy(text[lo:lo + m]))
        took = []
        for rep in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            N.check(lib.kbbq_bgzf_deflate_dev(ctx.handle, N.ptr(d_text), m, BLOCK, N.ptr(d_blocks), N.ptr(d_sizes), N.ptr(d_packed),
                                              ctypes.byref(total)))
            b.record()
            torch.cuda.synchronize()
            took.append(a.elapsed_time(b))
        ms += statistics.median(took[1:])
        packed += total.value
    result.update(kernel_ms=round(ms, 3), kernel_text_GB_per_s=round(text.size / ms / 1e6, 2), kernel_packed_bytes=packed + 28)
    assert result['kernel_packed_bytes'] == result['bgzf_bytes'], 'the file is not the blocks of the direct calls'
    say('sizes: zlib on the same cuts, %d threads' % args.threads)
    result.update(zlib_sizes(text))
    for key in ('bgzf_bytes', 'zlib_1', 'zlib_6', 'zlib_huffman_only'):
        result[key + '_ratio'] = round(result[key] / text.size, 4)
    for key in ('wall_plain_s', 'wall_bgzf_s', 'wall_gzip1_pipe_s'):
        if key in result:
            result[key] = round(result[key], 3)
    print(json.dumps(result), flush=True)
finally:
    for p in (fa, fb, fo, fz):
        if os.path.exists(p):
            os.remove(p)
