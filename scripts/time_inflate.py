#!/usr/bin/env python3
"""Measurements of the BGZF inflate on one GPU (csrc/kbbq_bgzf_inflate.h), on the FASTQ pair scripts/time_bgzf.py makes (`--reads`
synthetic 150-base reads, 8 M by default: 2.5 GB of text a file; written under TMPDIR and removed), each file compressed twice:
`own`, the project's own writer (kbbq_bgzf_deflate: what --bgzf writes), and `zlib6`, zlib level 6 on the same 65280-byte cuts.
  kernel   kbbq_inflate_bgzf_dev on device-resident slabs of file A (`--slab-blocks` members each), HIP events around the call,
           per slab the median of `--reps` after one warm-up; GB/s of text over the sum of the medians.
  open     the mapped reader on the pair (fastx.PairScan: map, inflate, index, scan), host route (KBBQ_GPU_INFLATE=0) against
           device route (KBBQ_GPU_INFLATE=1, a warm context), in turn, median of `--reps` after one warm-up each.
  wall     `kbbq recalibrate -f A.gz B.gz -o out` as a process, wall clock, in turn: `--parent ROOT` (a built checkout of the parent
           commit: THE comparison), this tree with KBBQ_GPU_INFLATE=0, this tree with KBBQ_GPU_INFLATE=1; median and spread
           (max - min) of `--reps` after one warm-up each; and the plain pair for scale.
Prints progress lines and one JSON line at the end.  usage (GPU box): python scripts/time_inflate.py [--reads N] [--parent ROOT]"""
import argparse
import concurrent.futures
import ctypes
import json
import os
import statistics
import struct
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
ap.add_argument('--parent', default=None, help='root of a built checkout of the parent commit')
args = ap.parse_args()

import numpy as np
import torch
from kbbq import _device as dev
from kbbq import _native as N
from kbbq import fastx

BLOCK = N.BGZF_BLOCK_MAX
HEAD = bytes.fromhex('1f8b08040000000000ff060042430200')
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
n = args.reads
tmp = os.environ.get('TMPDIR', '/tmp')
P = {k: os.path.join(tmp, 'kbbq_inflate_%d_%s' % (os.getpid(), k)) for k in
     ('a.fq', 'b.fq', 'a.own.fq.gz', 'b.own.fq.gz', 'a.zlib6.fq.gz', 'b.zlib6.fq.gz', 'out.fq')}


def say(*what):
    print(*what, flush=True)


def write_inputs():
    batch = dev.ReadBatch.synthetic(0, n, n, seed=1)
    seq, cseq, qual = (getattr(batch, p).cpu().numpy()[:n, :150] for p in ('seq', 'cseq', 'qual'))
    del batch
    for path, plane in ((P['a.fq'], seq), (P['b.fq'], cseq)):
        rec = np.empty((n, 318), dtype=np.uint8)
        ids = np.arange(n)
        rec[:, 0] = ord('@'); rec[:, 1] = ord('r'); rec[:, 11] = ord('/')
        rec[:, 2:11] = ((ids >> 1)[:, None] // 10 ** np.arange(8, -1, -1)[None, :] % 10 + 48).astype(np.uint8)
        rec[:, 12] = 49 + (ids & 1); rec[:, 13] = 10
        rec[:, 14:164] = plane; rec[:, 164] = 10; rec[:, 165] = ord('+'); rec[:, 166] = 10
        rec[:, 167:317] = qual; rec[:, 317] = 10
        rec.tofile(path)
        del rec


def compress(path, stem):
    lib, ctx = N.load(), dev.context()
    text = np.fromfile(path, dtype=np.uint8)
    bound = int(lib.kbbq_bgzf_bound(text.size, BLOCK))
    out, total = np.empty(bound, dtype=np.uint8), ctypes.c_size_t(0)
    N.check(lib.kbbq_bgzf_deflate(ctx.handle, N.ptr(text), text.size, BLOCK, N.ptr(out), bound, ctypes.byref(total)))
    with open(P[stem + '.own.fq.gz'], 'wb') as fh:
        fh.write(out[:total.value].tobytes() + EOF)

    def one(lo):
        piece = text[lo:lo + BLOCK].tobytes()
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        z = c.compress(piece) + c.flush()
        return HEAD + struct.pack('<H', len(z) + 25) + z + struct.pack('<II', zlib.crc32(piece), len(piece))
    with concurrent.futures.ThreadPoolExecutor(args.threads) as pool, open(P[stem + '.zlib6.fq.gz'], 'wb') as fh:
        for member in pool.map(one, range(0, text.size, BLOCK)):
            fh.write(member)
        fh.write(EOF)
    return text.size


def kernel_rate(path):
    lib, ctx = N.load(), dev.context()
    src = np.fromfile(path, dtype=np.uint8)
    nb, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    N.check(lib.kbbq_inflate_index(N.ptr(src), src.size, None, 0, ctypes.byref(nb), ctypes.byref(total)))
    blocks = (N.BgzfBlock * nb.value)()
    N.check(lib.kbbq_inflate_index(N.ptr(src), src.size, blocks, nb.value, ctypes.byref(nb), ctypes.byref(total)))
    table = np.frombuffer(blocks, dtype=np.uint64).reshape(-1, 4).copy()         # src, dst, csize | isize << 32, crc
    per = args.slab_blocks
    d_src = torch.empty(per * 65536, dtype=torch.uint8, device='cuda')
    d_out = torch.empty(per * 65536, dtype=torch.uint8, device='cuda')
    d_blocks = torch.empty(per * 32, dtype=torch.uint8, device='cuda')
    d_status = torch.empty(per, dtype=torch.int32, device='cuda')
    ms, refused = 0.0, 0
    for lo in range(0, nb.value, per):
        t = table[lo:lo + per].copy()
        m = len(t)
        base, obase = int(t[0, 0]), int(t[0, 1])
        comp = int(t[-1, 0]) + int(t[-1, 2] & 0xffffffff) - base
        text = int(t[-1, 1]) + int(t[-1, 2] >> 32) - obase
        t[:, 0] -= base; t[:, 1] -= obase
        d_src[:comp].copy_(torch.from_numpy(src[base:base + comp]))
        d_blocks[:m * 32].copy_(torch.from_numpy(t.view(np.uint8).reshape(-1)))
        took = []
        for rep in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            N.check(lib.kbbq_inflate_bgzf_dev(ctx.handle, N.ptr(d_src), comp, N.ptr(d_blocks), m, N.ptr(d_out), text, N.ptr(d_status)))
            b.record()
            torch.cuda.synchronize()
            took.append(a.elapsed_time(b))
        ms += statistics.median(took[1:])
        refused += int((d_status[:m] != 0).sum())
    return dict(ms=round(ms, 3), text_GB_per_s=round(total.value / ms / 1e6, 2), members=nb.value, refused=refused,
                ratio=round(src.size / total.value, 4))


def open_pair(za, zb, mode):
    os.environ['KBBQ_GPU_INFLATE'] = mode
    times = []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        A, B, _ = fastx.PairScan(za, zb, True).result()
        times.append(time.perf_counter() - t0)
        A.close(); B.close()
    os.environ.pop('KBBQ_GPU_INFLATE')
    return round(statistics.median(times[1:]), 4)


def wall(label, root, files, mode):
    env = dict(os.environ, PYTHONPATH=os.path.join(root, 'kbbq-py_amd'))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_GPU_INFLATE'):
        env.pop(var, None)
    if mode is not None:
        env['KBBQ_GPU_INFLATE'] = mode
    command = [sys.executable, '-m', 'kbbq.main', 'recalibrate', '-f', files[0], files[1], '-o', P['out.fq']]
    times = []
    for rep in range(args.reps + 1):
        if os.path.exists(P['out.fq']):
            os.remove(P['out.fq'])
        t0 = time.perf_counter()
        subprocess.run(command, check=True, env=env)
        times.append(time.perf_counter() - t0)
        say('  %s: repetition %d %.3f s' % (label, rep, times[-1]))
    return dict(median_s=round(statistics.median(times[1:]), 3), spread_s=round(max(times[1:]) - min(times[1:]), 3))


try:
    say('writing %d reads ...' % n)
    write_inputs()
    result = dict(reads=n, device=dev.context().name, reps=args.reps)
    result['text_bytes_a_file'] = compress(P['a.fq'], 'a')
    compress(P['b.fq'], 'b')
    for kind in ('own', 'zlib6'):
        za, zb = P['a.%s.fq.gz' % kind], P['b.%s.fq.gz' % kind]
        say('%s: kernel' % kind)
        r = dict(kernel=kernel_rate(za))
        say('%s: open' % kind)
        r['open_host_s'], r['open_device_s'] = open_pair(za, zb, '0'), open_pair(za, zb, '1')
        say('%s: wall' % kind)
        if args.parent:
            r['wall_parent'] = wall('parent', args.parent, (za, zb), None)
        r['wall_host'] = wall('host route', ROOT, (za, zb), '0')
        r['wall_device'] = wall('device route', ROOT, (za, zb), '1')
        result[kind] = r
    result['wall_plain'] = wall('plain pair', ROOT, (P['a.fq'], P['b.fq']), None)
    print(json.dumps(result), flush=True)
finally:
    for p in P.values():
        if os.path.exists(p):
            os.remove(p)
