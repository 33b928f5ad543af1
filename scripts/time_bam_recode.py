#!/usr/bin/env python3
"""What making the --bam-out skeleton on the GPU from resident BAM records (KBBQ_GPU_BAM=1: csrc/kbbq_bam_recode.h, kbbq/_bamin.py,
kbbq/_bamout.py) is worth for `kbbq applybqsr -b IN.bam -g R -s --bam-out -o OUT.bam`, on the set of profiles/bam_out.md:
`--pairs` pairs of 150-base reads with OQ tags (tests' oracle_bqsr.synth_bqsr_set), as a BAM file that `applybqsr --bam-out`
itself writes of the SAM text, and a report `kbbq bqsr` makes of them.
Every command is a process of its own; the host route (the variable unset) and the device route run alternating, one warm-up of
either, then `--reps` timed runs: wall time, peak host memory (ru_maxrss of the child), the route each took, and whether the two
files are the same bytes.  The recode alone by HIP events around kbbq_bam_recode_dev on the whole file as one range (5 warm-ups,
10 timed calls, median): bytes per second over the algorithmic bytes -- the record bytes, offsets and keep bytes read, the
descriptors, status words and skeleton written -- against the 8 TB/s HBM specification.  Prints one JSON line.
usage (GPU box): python scripts/time_bam_recode.py [--pairs 800000] [--reps 3] [--dir /tmp/x]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('kbbq-py_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))
ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=800_000)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--dir', default=None)
args = ap.parse_args()
HBM_SPEC = 8.0e12

RSS = ('import resource, sys\nsys.stderr.write("MAXRSS_KB %d\\n" % resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)\n')
COMMAND = ('import sys\nfrom kbbq import aln, main\nmain.main(sys.argv[1:])\nsys.stderr.write("ROUTE %s\\n" % aln.LAST_RUN.get("bam_in", {}).get("route"))\n'
           + RSS)
KERNEL = '''
import ctypes, json, sys
import numpy as np
import torch
from kbbq import _bamin as B, _device as dev, _native as N
T = dev._torch(); ctx = dev.context(); lib = N.load()
image = B.Image(sys.argv[1]); raw = image.bytes; scan = B.Scan(raw)
n, lo = scan.n, scan.records_off
up = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
d_stream = up(raw[lo:])
d_rec = up((scan.rec_off.astype(np.int64) - lo))
cap = scan.stream_bytes + n * (scan.maxlen + 4)
d_desc = T.empty(24 * n, dtype=T.uint8, device='cuda'); d_status = T.empty(n, dtype=T.int32, device='cuda')
d_skel = T.empty(cap, dtype=T.uint8, device='cuda')
sb, tb, st = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0)
out = {}
for set_oq in (0, 1):
    def call():
        N.check(lib.kbbq_bam_recode_dev(ctx.handle, N.ptr(d_stream), scan.stream_bytes, N.ptr(d_rec), 0, n, set_oq, None, scan.n_ref, N.ptr(d_desc),
                                        N.ptr(d_skel), cap, N.ptr(d_status), ctypes.byref(sb), ctypes.byref(tb), ctypes.byref(st)))
    ms = []
    for i in range(15):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); b.synchronize()
        if i >= 5:
            ms.append(a.elapsed_time(b))
    algorithmic = scan.stream_bytes + 8 * n + 24 * n + 4 * n + sb.value
    out['set_oq=%d' % set_oq] = dict(ms=sorted(round(x, 4) for x in ms), median_ms=round(float(np.median(ms)), 4), status=st.value, records=n,
                                     stream_bytes=scan.stream_bytes, skeleton_bytes=sb.value, out_stream_bytes=tb.value,
                                     algorithmic_bytes=algorithmic)
print('KERNEL ' + json.dumps(out))
'''


def child(argv, device):
    """(wall seconds, stdout, stderr) of one process."""
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_GPU_BAM'):
        env.pop(var, None)
    if device:
        env['KBBQ_GPU_BAM'] = '1'
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable] + argv, env=env, capture_output=True, timeout=1200)
    wall = time.perf_counter() - t0
    if p.returncode:
        sys.exit('%s failed (%d):\n%s' % (' '.join(argv[:1] + argv[2:]), p.returncode, p.stderr.decode('utf-8', 'replace')[-3000:]))
    return wall, p.stdout.decode(), p.stderr.decode('utf-8', 'replace')


def main():
    import oracle_bqsr as OQ
    tmp = args.dir or tempfile.mkdtemp(prefix='kbbq-time-bam-recode-', dir=os.environ.get('TMPDIR'))
    os.makedirs(tmp, exist_ok=True)
    try:
        t0 = time.perf_counter()
        paths = OQ.synth_bqsr_set(tmp, seed=1, npairs=args.pairs, S=150, contigs=(('chr1', 3_000_000), ('chr2', 1_000_000)))
        report, bam = os.path.join(tmp, 'model.grp'), os.path.join(tmp, 'in.bam')
        child(['-c', COMMAND, 'bqsr', '-b', paths['sam'], '-r', paths['fa'], '-v', paths['vcf'], '-g', report], False)
        # the input BAM: the records as read, written by --bam-out itself with a model that changes nothing of what is timed
        child(['-c', COMMAND, 'applybqsr', '-b', paths['sam'], '-g', report, '--bam-out', '-o', bam], False)
        os.unlink(paths['sam'])
        res = dict(alignments=2 * args.pairs, reps=args.reps, bam_bytes=os.path.getsize(bam), write_set_s=round(time.perf_counter() - t0, 1))
        print('set written: %s' % json.dumps(res), flush=True)
        out = {False: os.path.join(tmp, 'host.bam'), True: os.path.join(tmp, 'device.bam')}

        def command(device):
            if os.path.exists(out[device]):
                os.remove(out[device])
            w, _, err = child(['-c', COMMAND, 'applybqsr', '-b', bam, '-g', report, '-s', '--bam-out', '-o', out[device]], device)
            route = err.rsplit('ROUTE ', 1)[1].split()[0]
            assert route == ('device' if device else 'host'), err[-2000:]
            print('  %s route: %.3f s' % (route, w), flush=True)
            return w, round(int(err.rsplit('MAXRSS_KB ', 1)[1].split()[0]) / 1024.0, 1)
        command(False); command(True)                                    # the warm-up: page cache, code objects on disk
        runs = {False: [], True: []}
        for _ in range(args.reps):
            for device in (False, True):
                runs[device].append(command(device))
        res['same_file'] = open(out[False], 'rb').read() == open(out[True], 'rb').read()
        res['out_bytes'] = os.path.getsize(out[True])
        for device, name in ((False, 'host'), (True, 'device')):
            res[name] = dict(wall_s=round(float(np.median([r[0] for r in runs[device]])), 3), wall_all=[round(r[0], 3) for r in runs[device]],
                             peak_rss_mb=round(float(np.median([r[1] for r in runs[device]])), 1), peak_rss_all=[r[1] for r in runs[device]])
        _, kout, _ = child(['-c', KERNEL, bam], True)
        k = json.loads(kout.rsplit('KERNEL ', 1)[1])
        for v in k.values():
            v['algorithmic_bytes_per_s'] = round(v['algorithmic_bytes'] / (v['median_ms'] * 1e-3))
            v['share_of_hbm_spec'] = round(v['algorithmic_bytes_per_s'] / HBM_SPEC, 4)
        res['recode'] = k
        print(json.dumps(res), flush=True)
    finally:
        if not args.dir:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
