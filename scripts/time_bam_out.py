#!/usr/bin/env python3
"""Measurements of --bam-out on one GPU, on the alignments tests/tools/time_sam_paths.py generates (`--pairs` pairs of 150-base
reads with OQ tags, written under TMPDIR and removed) and a report `kbbq bqsr` makes of them.
  wall       `kbbq applybqsr -b ALN -g R -s -o OUT` as a process, wall clock, median of `--reps` after one warm-up round, a fresh
             output file each time: plain SAM, --bgzf (the SAM text deflated on the GPU) and --bam-out, run in turn.  The --bam-out file must
             inflate to tests/bamwriter.py's encoding of the plain output (checked on the first `--check` alignments' bytes).
  stages     in this process, on the whole file as one slab: the host passes (kbbq_bam_check, kbbq_bam_layout, kbbq_bam_skeleton),
             the upload of skeleton and descriptors, kbbq_bam_assemble_dev (HIP events around the call, median of `--reps` after
             one warm-up) and kbbq_bgzf_deflate_dev over the assembled stream in slabs of 256 blocks.
  kernel     the assemble call's GB/s of stream, and its algorithmic bytes -- descriptors, skeleton, SEQ and QUAL characters read,
             stream written -- per second as a fraction of the HBM specification (8 TB/s).
Prints progress lines and one JSON line at the end.  usage (GPU box): python scripts/time_bam_out.py [--pairs N]"""
import argparse
import ctypes
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('kbbq-py_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))
ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=250_000)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--check', type=int, default=20_000, help='alignments whose bytes are compared with bamwriter (0: all)')
args = ap.parse_args()

import numpy as np
import torch
import oracle_bqsr as OQ
from kbbq import _device as dev
from kbbq import _native as N
from kbbq import aln

HBM_SPEC = 8.0e12
BLOCK = N.BGZF_BLOCK_MAX
tmp = tempfile.mkdtemp(prefix='kbbq_bam_out_', dir=os.environ.get('TMPDIR'))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH'):
    ENV.pop(var, None)


def say(*what):
    print(*what, flush=True)


def walls(variants):
    """{key: (median, runs, output bytes)} of the commands of `variants` [(key, label, command, out)], run in turn `--reps` + 1
    times -- the variants alternate, so that what else the host does falls on all of them -- the first round being the warm-up."""
    times = {key: [] for key, _, _, _ in variants}
    for rep in range(args.reps + 1):
        for key, label, command, out in variants:
            if os.path.exists(out):
                os.remove(out)               # a fresh output file: truncating the page cache is not the command's time
            t0 = time.perf_counter()
            subprocess.run(command, check=True, env=ENV)
            times[key].append(time.perf_counter() - t0)
            say('  %s: repetition %d %.3f s, %d bytes' % (label, rep, times[key][-1], os.path.getsize(out)))
    return {key: (round(statistics.median(times[key][1:]), 3), [round(t, 3) for t in times[key][1:]], os.path.getsize(out))
            for key, _, _, out in variants}


def timed(fn):
    t0 = time.perf_counter()
    value = fn()
    return value, time.perf_counter() - t0


try:
    t0 = time.perf_counter()
    paths = OQ.synth_bqsr_set(tmp, seed=1, npairs=args.pairs, S=150, contigs=(('chr1', 3_000_000), ('chr2', 1_000_000)))
    sam, report = paths['sam'], os.path.join(tmp, 'model.grp')
    say('generated %d alignments in %.1f s (%.1f MB of SAM)' % (2 * args.pairs, time.perf_counter() - t0, os.path.getsize(sam) / 1e6))
    kbbq = [sys.executable, '-m', 'kbbq.main']
    subprocess.run(kbbq + ['bqsr', '-b', sam, '-r', paths['fa'], '-v', paths['vcf'], '-g', report], check=True, env=ENV)
    result = dict(alignments=2 * args.pairs, device=dev.context().name, reps=args.reps, input_bytes=os.path.getsize(sam))
    apply = kbbq + ['applybqsr', '-b', sam, '-g', report, '-s']
    outs = {k: os.path.join(tmp, 'out.' + k) for k in ('sam', 'sam.gz', 'bam')}
    say('wall: applybqsr -s, plain SAM / --bgzf / --bam-out in turn')
    measured = walls([('plain', 'plain SAM', apply + ['-o', outs['sam']], outs['sam']),
                      ('bgzf', '--bgzf', apply + ['--bgzf', '-o', outs['sam.gz']], outs['sam.gz']),
                      ('bam_out', '--bam-out', apply + ['--bam-out', '-o', outs['bam']], outs['bam'])])
    for key, (median, runs, size) in measured.items():
        result['wall_%s_s' % key], result['wall_%s_runs' % key], result['%s_bytes' % key] = median, runs, size
    # the file is the stream the plain output defines
    import bamwriter
    with open(outs['sam'], 'rb') as fh:
        text = fh.read().decode('latin-1')
    lines = text.split('\n')
    head = sum(1 for ln in lines if ln.startswith('@'))
    some = lines[:head + (args.check or len(lines))]
    want = bamwriter.sam_to_bam_bytes('\n'.join(some) + '\n')
    with gzip.open(outs['bam'], 'rb') as fh:
        stream = fh.read()
    assert stream[:len(want)] == want, 'the --bam-out file is not the BAM encoding of the plain output'
    result.update(text_bytes=len(text), stream_bytes=len(stream), stream_of_text=round(len(stream) / len(text), 4))
    del text, lines, some, want

    say('stages: one slab of %d alignments' % (2 * args.pairs))
    lib, ctx = N.load(), dev.context()
    bam, parse_s = timed(lambda: aln.AlignmentFile(sam))
    b, n = bam.batch(), len(bam)
    pitch = max(16, (int(b.maxlen) + 15) // 16 * 16)
    bad = ctypes.c_int64(-1)
    _, check_s = timed(lambda: N.check(lib.kbbq_bam_check(b._native, 0, n, ctypes.byref(bad))))
    desc = np.empty((n, N.BAM_DESC_WORDS), dtype=np.uint32)
    skel_bytes, stream_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _, layout_s = timed(lambda: N.check(lib.kbbq_bam_layout(b._native, 0, n, 1, None, N.ptr(desc), ctypes.byref(skel_bytes),
                                                            ctypes.byref(stream_bytes))))
    skel = torch.empty(skel_bytes.value, dtype=torch.uint8, pin_memory=True)
    _, skeleton_s = timed(lambda: N.check(lib.kbbq_bam_skeleton(b._native, 0, n, 1, N.ptr(desc), N.ptr(skel), skel_bytes.value)))
    torch.cuda.synchronize()
    (d_skel, d_desc), upload_s = timed(lambda: (skel.cuda(), torch.from_numpy(desc.view(np.int32)).cuda(), torch.cuda.synchronize())[:2])
    d_seq = torch.from_numpy(b.plane(0, pitch)).cuda()
    d_out = torch.from_numpy(b.plane(1, pitch)).cuda()               # QUAL as read stands in for the apply's output plane
    d_stream = torch.empty(stream_bytes.value + 16, dtype=torch.uint8, device='cuda')
    took = []
    for rep in range(args.reps + 1):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        N.check(lib.kbbq_bam_assemble_dev(ctx.handle, N.ptr(d_skel), skel_bytes.value, N.ptr(d_desc), n, N.ptr(d_seq), N.ptr(d_out), pitch,
                                          N.ptr(d_stream), 0, stream_bytes.value, ctypes.byref(bad)))
        e.record()
        torch.cuda.synchronize()
        took.append(a.elapsed_time(e))
    assert bad.value == -1
    assemble_ms = statistics.median(took[1:])
    lens = b.qlen.astype(np.int64)
    algorithmic = desc.nbytes + skel_bytes.value + 2 * int(lens.sum()) + stream_bytes.value
    slab = 256 * BLOCK
    d_blocks = torch.empty(256 * N.BGZF_SLOT, dtype=torch.uint8, device='cuda')
    d_sizes = torch.empty(256, dtype=torch.int32, device='cuda')
    d_packed = torch.empty(int(lib.kbbq_bgzf_bound(slab, BLOCK)), dtype=torch.uint8, device='cuda')
    total, packed = ctypes.c_size_t(0), 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for lo in range(0, stream_bytes.value, slab):
        N.check(lib.kbbq_bgzf_deflate_dev(ctx.handle, N.ptr(d_stream.data_ptr() + lo), min(slab, stream_bytes.value - lo), BLOCK,
                                          N.ptr(d_blocks), N.ptr(d_sizes), N.ptr(d_packed), ctypes.byref(total)))
        packed += total.value
    deflate_s = time.perf_counter() - t0
    result.update(parse_s=round(parse_s, 3), check_s=round(check_s, 3), layout_s=round(layout_s, 3), skeleton_s=round(skeleton_s, 3),
                  upload_s=round(upload_s, 4), skeleton_bytes=skel_bytes.value, descriptor_bytes=desc.nbytes,
                  record_stream_bytes=stream_bytes.value, assemble_ms=round(assemble_ms, 3), assemble_runs_ms=[round(t, 3) for t in took[1:]],
                  assemble_stream_GB_per_s=round(stream_bytes.value / assemble_ms / 1e6, 1),
                  assemble_algorithmic_bytes=algorithmic,
                  assemble_of_hbm_spec=round(algorithmic / (assemble_ms / 1e3) / HBM_SPEC, 4),
                  deflate_s=round(deflate_s, 3), deflate_stream_GB_per_s=round(stream_bytes.value / deflate_s / 1e9, 2),
                  deflated_bytes=packed)
    print(json.dumps(result), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
