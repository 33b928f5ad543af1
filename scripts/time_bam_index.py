#!/usr/bin/env python3
"""Measurements of --bam-index on one GPU, on the alignments scripts/time_bam_out.py uses (`--pairs` pairs of 150-base reads with OQ
tags), sorted by coordinate -- an index needs that -- written under TMPDIR and removed, and a report `kbbq bqsr` makes of them.
  wall       `kbbq applybqsr -b ALN -g R -s --bam-out -o OUT` as a process, wall clock, median of `--reps` after one warm-up round,
             fresh output files each time: without the option and with --bam-index, run in turn; with `--parent DIR` (the
             kbbq-py_amd directory of a build of the parent commit) the parent's command runs in the same rounds.  The BAM of the
             run with the option must be the one without it, byte for byte; the index is parsed and its counts are checked.
  kernel     in this process, the whole file as one slab: kbbq_bam_index_dev (HIP events around the call: the five kernels, the
             words and the runs coming back), median of `--reps` after one warm-up; the runs and their bytes.
  stages     with `--stages`: one more run with the option under KBBQ_TIMING=1, its stderr passed on.
Prints progress lines and one JSON line at the end.  usage (GPU box): python scripts/time_bam_index.py [--pairs N] [--parent DIR]"""
import argparse
import ctypes
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
ap.add_argument('--parent', default=None, help='kbbq-py_amd of a build of the parent commit: its --bam-out runs in turn with this one\'s')
ap.add_argument('--stages', action='store_true')
args = ap.parse_args()

import numpy as np
import torch
import oracle_bqsr as OQ
import bam_index_model as M
from kbbq import _bamindex
from kbbq import _device as dev
from kbbq import _native as N
from kbbq import aln

tmp = tempfile.mkdtemp(prefix='kbbq_bam_index_', dir=os.environ.get('TMPDIR'))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH'):
    ENV.pop(var, None)


def say(*what):
    print(*what, flush=True)


def walls(variants):
    """{key: (median, runs)} of the commands of `variants` [(key, label, command, env, outputs)], run in turn `--reps` + 1 times,
    the first round being the warm-up."""
    times = {key: [] for key, *_ in variants}
    for rep in range(args.reps + 1):
        for key, label, command, env, outs in variants:
            for out in outs:
                if os.path.exists(out):
                    os.remove(out)           # fresh output files: truncating the page cache is not the command's time
            t0 = time.perf_counter()
            subprocess.run(command, check=True, env=env)
            times[key].append(time.perf_counter() - t0)
            say('  %s: repetition %d %.3f s' % (label, rep, times[key][-1]))
    return {key: (round(statistics.median(times[key][1:]), 3), [round(t, 3) for t in times[key][1:]]) for key in times}


try:
    t0 = time.perf_counter()
    paths = OQ.synth_bqsr_set(tmp, seed=1, npairs=args.pairs, S=150, contigs=(('chr1', 3_000_000), ('chr2', 1_000_000)))
    with open(paths['sam']) as fh:
        lines = fh.read().split('\n')
    header = [ln for ln in lines if ln.startswith('@')]
    order = {ln.split('\t')[1][3:]: k for k, ln in enumerate(ln for ln in header if ln.startswith('@SQ'))}
    order['*'] = len(order)
    records = [ln for ln in lines if ln and not ln.startswith('@')]
    keys = [(order[f[2]], int(f[3])) for f in (ln.split('\t', 4) for ln in records)]
    records = [records[k] for k in sorted(range(len(records)), key=keys.__getitem__)]
    sam = os.path.join(tmp, 'sorted.sam')
    with open(sam, 'w') as fh:
        fh.write('\n'.join(header + records) + '\n')
    del lines, records, keys
    report = os.path.join(tmp, 'model.grp')
    say('generated and sorted %d alignments in %.1f s (%.1f MB of SAM)' % (2 * args.pairs, time.perf_counter() - t0, os.path.getsize(sam) / 1e6))
    kbbq = [sys.executable, '-m', 'kbbq.main']
    subprocess.run(kbbq + ['bqsr', '-b', sam, '-r', paths['fa'], '-v', paths['vcf'], '-g', report], check=True, env=ENV)
    result = dict(alignments=2 * args.pairs, device=dev.context().name, reps=args.reps, input_bytes=os.path.getsize(sam))
    apply = kbbq + ['applybqsr', '-b', sam, '-g', report, '-s', '--bam-out']
    outs = {k: os.path.join(tmp, k + '.bam') for k in ('parent', 'plain', 'index')}
    variants = []
    if args.parent:
        variants.append(('parent', 'parent commit, --bam-out', apply + ['-o', outs['parent']], dict(ENV, PYTHONPATH=args.parent), [outs['parent']]))
    variants += [('plain', '--bam-out', apply + ['-o', outs['plain']], ENV, [outs['plain']]),
                 ('index', '--bam-out --bam-index', apply + ['--bam-index', '-o', outs['index']], ENV, [outs['index'], outs['index'] + '.bai'])]
    say('wall: applybqsr -s --bam-out, %s in turn' % ' / '.join(label for _, label, *_ in variants))
    for key, (median, runs) in walls(variants).items():
        result['wall_%s_s' % key], result['wall_%s_runs' % key] = median, runs
    with open(outs['index'], 'rb') as a, open(outs['plain'], 'rb') as b:
        assert a.read() == b.read(), 'the BAM written with --bam-index differs from the one without'
    if args.parent:
        with open(outs['parent'], 'rb') as a, open(outs['plain'], 'rb') as b:
            assert a.read() == b.read(), 'the BAM differs from the parent commit\'s'
    with open(outs['index'] + '.bai', 'rb') as fh:
        index = M.parse(fh.read())
    counted = index['n_no_coor'] + sum(entry['meta'][2] + entry['meta'][3] for entry in index['refs'] if entry['meta'])
    assert counted == 2 * args.pairs, 'the index counts %d alignments' % counted
    result.update(bam_bytes=os.path.getsize(outs['index']), index_bytes=os.path.getsize(outs['index'] + '.bai'),
                  index_bins=sum(len(entry['bins']) for entry in index['refs']),
                  index_chunks=sum(len(c) for entry in index['refs'] for c in entry['bins'].values()))
    if args.stages:
        say('stages: KBBQ_TIMING=1, with --bam-index')
        subprocess.run(apply + ['--bam-index', '-o', outs['index']], check=True, env=dict(ENV, KBBQ_TIMING='1'))

    say('kernel: one slab of %d alignments' % (2 * args.pairs))
    lib, ctx = N.load(), dev.context()
    bam = aln.AlignmentFile(sam)
    b, n = bam.batch(), len(bam)
    t0 = time.perf_counter()
    _bamindex.check(bam, 5)
    result['check_s'] = round(time.perf_counter() - t0, 4)
    desc = np.empty((n, N.BAM_DESC_WORDS), dtype=np.uint32)
    skel_bytes, stream_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
    N.check(lib.kbbq_bam_layout(b._native, 0, n, 1, None, N.ptr(desc), ctypes.byref(skel_bytes), ctypes.byref(stream_bytes)))
    skel = np.empty(skel_bytes.value, dtype=np.uint8)
    N.check(lib.kbbq_bam_skeleton(b._native, 0, n, 1, N.ptr(desc), N.ptr(skel), skel_bytes.value))
    d_skel, d_desc = torch.from_numpy(skel).cuda(), torch.from_numpy(desc.view(np.int32)).cuda()
    made = _bamindex.Index('bai', 5, [ln for _, ln, _ in _bamindex.references(bam.header)])
    d_lin_off = torch.from_numpy(made.lin_off.view(np.int64)).cuda()
    windows = int(made.lin_off[-1])
    runs = np.empty(n * N.BAM_RUN_BYTES, dtype=np.uint8)
    count, bad = ctypes.c_int64(0), ctypes.c_int64(-1)
    took = []
    for rep in range(args.reps + 1):
        d_linear = torch.full((windows,), -1, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        N.check(lib.kbbq_bam_index_dev(ctx.handle, N.ptr(d_skel), skel_bytes.value, N.ptr(d_desc), n, 0, 5, N.ptr(d_lin_off), made.n_ref,
                                       N.ptr(d_linear), N.ptr(runs), n, ctypes.byref(count), ctypes.byref(bad)))
        e.record()
        torch.cuda.synchronize()
        took.append(a.elapsed_time(e))
    assert bad.value == -1
    n_cigar = int(b.cig_n.astype(np.int64).sum())
    read = desc.nbytes + 36 * n + 4 * n_cigar                        # descriptors, the fixed fields, the CIGAR words
    result.update(index_ms=round(statistics.median(took[1:]), 3), index_runs_ms=[round(t, 3) for t in took[1:]], runs=count.value,
                  runs_bytes=count.value * N.BAM_RUN_BYTES, linear_bytes=8 * windows, bytes_read_per_record=round(read / n, 1))
    print(json.dumps(result), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
