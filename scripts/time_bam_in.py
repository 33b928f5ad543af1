#!/usr/bin/env python3
"""What decoding BAM records on the GPU (KBBQ_GPU_BAM=1: csrc/kbbq_bam_in.h, kbbq/_bamin.py) is worth for `kbbq bqsr --kmers -g`,
on the set of profiles/recalibrate_bam.md (scripts/time_recalibrate_bam.py writes it: `--reads` alignments of `--len` bases as BAM).
Every command is a process of its own; the host route (the variable unset, from `--parent-tree DIR`: a checkout of the parent
commit with its library built -- or from this tree, which launches the same without the variable) and the device route run
alternating, one warm-up of either, then `--reps` timed runs: wall time, peak host memory (ru_maxrss of the child), and whether
the reports are the same bytes.  The parse stage -- `bqsr` prints no stage lines -- is the time of aln.alignments(path) + batch()
in a child that opens the file twice (the first open pays the library load and, on the device route, the context).  The kernel
alone by HIP events around kbbq_bam_decode_dev on the whole stream as one resident slab (5 warm-ups, 10 timed calls, median):
bytes per second over the algorithmic bytes -- the record bytes and offset tables read, the planes, words and CIGAR words written
-- against the 8 TB/s HBM specification.  Prints one JSON line.
usage (GPU box): python scripts/time_bam_in.py [--reads 2000000] [--len 150] [--dir /tmp/x] [--parent-tree DIR]"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=2_000_000)
ap.add_argument('--len', type=int, default=150)
ap.add_argument('-k', type=int, default=31)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--dir', default=None)
ap.add_argument('--parent-tree', default=None)
args = ap.parse_args()
HBM_SPEC = 8.0e12


def write_set(tmp):
    """aln.bam by the generator of scripts/time_recalibrate_bam.py (the module reads its options from sys.argv when it is loaded)."""
    keep = sys.argv
    sys.argv = ['time_recalibrate_bam.py', '--reads', str(args.reads), '--len', str(args.len)]
    try:
        spec = importlib.util.spec_from_file_location('time_recalibrate_bam', os.path.join(ROOT, 'scripts', 'time_recalibrate_bam.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv = keep
    sam, bam = os.path.join(tmp, 'aln.sam'), os.path.join(tmp, 'aln.bam')
    mod.write_set(sam, bam)
    os.unlink(sam)
    return bam


def child(argv, tree, device):
    """(wall seconds, peak resident MB, stdout, stderr) of one process."""
    env = dict(os.environ, PYTHONPATH=os.path.join(tree, 'kbbq-py_amd'))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_GPU_BAM'):
        env.pop(var, None)
    if device:
        env['KBBQ_GPU_BAM'] = '1'
    t0 = time.perf_counter()
    p = subprocess.Popen([sys.executable] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.communicate(timeout=1200)
    wall = time.perf_counter() - t0
    _, status, usage = os.wait4(p.pid, 0) if p.returncode is None else (0, p.returncode, None)
    if p.returncode:
        sys.exit('%s failed (%d):\n%s' % (' '.join(argv), p.returncode, err.decode('utf-8', 'replace')[-3000:]))
    return wall, usage, out.decode(), err.decode('utf-8', 'replace')


RSS = ('import resource, sys\nsys.stderr.write("MAXRSS_KB %d\\n" % resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)\n')
COMMAND = 'import sys\nfrom kbbq import main\nmain.main(sys.argv[1:])\n' + RSS
OPEN = ('import sys, time\nfrom kbbq import aln\nout = []\n'
        'for _ in range(2):\n    t0 = time.perf_counter()\n    b = aln.alignments(sys.argv[1]) if hasattr(aln, "alignments") else aln.AlignmentFile(sys.argv[1])\n'
        '    n = b.batch().n\n    out.append(time.perf_counter() - t0)\n    route = getattr(aln, "LAST_RUN", {}).get("bam_in", {}).get("route", "host")\n    del b\n'
        'print("OPEN %.4f %.4f %s %d" % (out[0], out[1], route, n))\n' + RSS)
KERNEL = '''
import ctypes, json, sys
import numpy as np
import torch
from kbbq import _bamin as B, _device as dev, _native as N
T = dev._torch(); ctx = dev.context(); lib = N.load()
image = B.Image(sys.argv[1]); raw = image.bytes; scan = B.Scan(raw)
n, pitch = scan.n, max(16, (scan.maxlen + 15) // 16 * 16)
lo = scan.records_off
rec, cig = B._slab_tables(scan, 0, n, lo)
up = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
d_slab, d_rec, d_cig = up(raw[lo:]), up(rec.view(np.int32)), up(cig.view(np.int32))
d_rg_off, d_rg = up(scan.rg_off.view(np.int32)), up(scan.rg_bytes)
planes = [T.empty((n, pitch), dtype=T.uint8, device='cuda') for _ in range(3)]
words = T.empty((n, 16), dtype=T.int32, device='cuda'); ops = T.empty(max(scan.cig_total, 1), dtype=T.int32, device='cuda')
st = ctypes.c_uint32(0)
def call():
    N.check(lib.kbbq_bam_decode_dev(ctx.handle, N.ptr(d_slab), raw.nbytes - lo, N.ptr(d_rec), n, pitch, N.ptr(d_rg_off), N.ptr(d_rg), len(scan.rg_ids),
                                    scan.n_ref, N.ptr(d_cig), scan.cig_total, *[N.ptr(p) for p in planes], N.ptr(words), N.ptr(ops), ctypes.byref(st)))
ms = []
for i in range(15):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); call(); b.record(); b.synchronize()
    if i >= 5:
        ms.append(a.elapsed_time(b))
algorithmic = (raw.nbytes - lo) + rec.nbytes + cig.nbytes + 3 * n * pitch + 64 * n + 4 * scan.cig_total
print('KERNEL ' + json.dumps(dict(ms=sorted(round(x, 4) for x in ms), median_ms=round(float(np.median(ms)), 4), status=st.value, records=n, pitch=pitch,
                                  stream_bytes=raw.nbytes - lo, algorithmic_bytes=algorithmic)))
'''


def rss_mb(err):
    return round(int(err.rsplit('MAXRSS_KB ', 1)[1].split()[0]) / 1024.0, 1)


def main():
    tmp = args.dir or tempfile.mkdtemp(prefix='kbbq-time-bam-in-')
    os.makedirs(tmp, exist_ok=True)
    t0 = time.perf_counter()
    bam = write_set(tmp)
    host_tree = args.parent_tree or ROOT
    res = dict(reads=args.reads, len=args.len, k=args.k, reps=args.reps, bam_bytes=os.path.getsize(bam), write_set_s=round(time.perf_counter() - t0, 1),
               host_route_from='the parent tree given' if args.parent_tree else 'this tree, the variable unset')
    grp = {False: os.path.join(tmp, 'host.grp'), True: os.path.join(tmp, 'device.grp')}

    def command(device):
        w, _, _, err = child(['-c', COMMAND, 'bqsr', '--kmers', '-k', str(args.k), '-b', bam, '-g', grp[device]], ROOT if device else host_tree, device)
        return w, rss_mb(err)

    def opened(device):
        _, _, out, err = child(['-c', OPEN, bam], ROOT if device else host_tree, device)
        first, second, route, n = out.rsplit('OPEN ', 1)[1].split()
        assert route == ('device' if device else 'host') and int(n) == args.reads, out
        return float(first), float(second), rss_mb(err)
    command(False); command(True)                                    # the warm-up: page cache, code objects on disk
    runs = {False: [], True: []}
    opens = {False: [], True: []}
    for _ in range(args.reps):
        for device in (False, True):
            runs[device].append(command(device))
            opens[device].append(opened(device))
    res['same_report'] = open(grp[False], 'rb').read() == open(grp[True], 'rb').read()
    for device, name in ((False, 'host'), (True, 'device')):
        res[name] = dict(wall_s=round(float(np.median([r[0] for r in runs[device]])), 3), wall_all=[round(r[0], 3) for r in runs[device]],
                         peak_rss_mb=round(float(np.median([r[1] for r in runs[device]])), 1), peak_rss_all=[r[1] for r in runs[device]],
                         open_first_s=round(float(np.median([o[0] for o in opens[device]])), 3), open_first_all=[round(o[0], 3) for o in opens[device]],
                         open_second_s=round(float(np.median([o[1] for o in opens[device]])), 3), open_second_all=[round(o[1], 3) for o in opens[device]],
                         open_peak_rss_mb=round(float(np.median([o[2] for o in opens[device]])), 1))
    _, _, out, _ = child(['-c', KERNEL, bam], ROOT, True)
    k = json.loads(out.rsplit('KERNEL ', 1)[1])
    k['algorithmic_bytes_per_s'] = round(k['algorithmic_bytes'] / (k['median_ms'] * 1e-3))
    k['share_of_hbm_spec'] = round(k['algorithmic_bytes_per_s'] / HBM_SPEC, 3)
    res['kernel'] = k
    print(json.dumps(res))


if __name__ == '__main__':
    main()
