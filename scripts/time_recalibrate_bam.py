#!/usr/bin/env python3
"""Wall time of `kbbq recalibrate -b ALN --kmers -o OUT` against the two commands it stands for, `kbbq bqsr -b ALN --kmers -g R`
then `kbbq applybqsr -b ALN -g R -o OUT`, as processes of their own on one synthetic set: `--reads` alignments of `--len`
bases, one query length, sampled from a random genome sized for `--depth` x coverage with `--err` uniform substitutions, half of
them reverse-strand records, two read groups, qualities 2..41 -- written once as SAM text and as BAM (BGZF level 1) under
`--dir`.  Per file: one warm-up of either form, then `--reps` timed runs of either, alternating; the median wall times, the
stage times KBBQ_TIMING=1 prints for every command (median per stage), `h2d_plane_bytes` of the one run (its planes, n x pitch
each) beside the planes the two commands fill and upload between them, and whether the outputs and the reports are the same
bytes.  `--two-commands-tree DIR`: take the two commands from the package under DIR (a checkout of the parent commit with its
library built) instead of this tree's.  Prints one JSON line.
usage (GPU box): python scripts/time_recalibrate_bam.py [--reads 2000000] [--len 150] [--dir /tmp/x] [--two-commands-tree DIR]"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=2_000_000)
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--depth', type=float, default=30.0)
ap.add_argument('--err', type=float, default=0.01)
ap.add_argument('-k', type=int, default=31)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--dir', default=None)
ap.add_argument('--two-commands-tree', default=None)
ap.add_argument('--threads', type=int, default=min(16, os.cpu_count() or 1))
args = ap.parse_args()
n, L = args.reads, args.len
assert L % 2 == 0 and n < 10 ** 8
G = max(int(n * L / args.depth), 10 * L)
lo_pos = 10 ** len(str(G))                        # every POS has the same number of digits: fixed-width records
contig_len = lo_pos + G + L
rng = np.random.default_rng(5)


def digits(values, width):
    """[len(values), width] ASCII digits, zero padded (used for fields whose values all have `width` digits, and for names)."""
    v = np.asarray(values, dtype=np.int64)
    out = np.empty((v.shape[0], width), dtype=np.uint8)
    for j in range(width - 1, -1, -1):
        out[:, j] = 48 + v % 10
        v = v // 10
    return out


def make(chunk=1 << 18):
    """Yields (seq letters [m, L], qual characters [m, L], pos0 [m], reverse [m], read group [m]) chunk by chunk."""
    genome = rng.integers(0, 4, G, dtype=np.uint8)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    col = np.arange(L)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        start = rng.integers(0, G - L + 1, m)
        b = genome[start[:, None] + col]
        err = rng.random((m, L)) < args.err
        b = np.where(err, (b + rng.integers(1, 4, (m, L), dtype=np.uint8)) % 4, b).astype(np.uint8)
        yield lo, acgt[b], rng.integers(35, 75, (m, L), dtype=np.uint8), start + lo_pos, rng.random(m) < 0.5, rng.integers(0, 2, m)


HEADER = '@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:%d\n@RG\tID:g0\tPU:unit0\tSM:s\n@RG\tID:g1\tPU:unit1\tSM:s\n' % contig_len


def reg2bin(beg, end):
    end = end - 1
    out = np.zeros(beg.shape, dtype=np.int64)
    done = np.zeros(beg.shape, dtype=bool)
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        hit = ~done & ((beg >> shift) == (end >> shift))
        out[hit] = base + (beg[hit] >> shift)
        done |= hit
    return out


def bgzf(data, pool, block=0xff00):
    def one(at):
        chunk = data[at:at + block]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff' + struct.pack('<H', 6) + b'BC' + struct.pack('<HH', 2, 18 + len(comp) + 8 - 1)
                + comp + struct.pack('<II', zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return b''.join(pool.map(one, range(0, len(data), block)))


def write_set(sam_path, bam_path):
    pw = len(str(lo_pos))
    code = np.zeros(256, dtype=np.uint8)
    for i, c in enumerate(b'=ACMGRSVTWYHKDBN'):
        code[c] = i
    with open(sam_path, 'wb') as sam, open(bam_path, 'wb') as bam, ThreadPoolExecutor(args.threads) as pool:
        sam.write(HEADER.encode())
        htext = HEADER.encode()
        bam.write(bgzf(b'BAM\1' + struct.pack('<i', len(htext)) + htext + struct.pack('<i', 1) + struct.pack('<i', 5) + b'chr1\0'
                       + struct.pack('<i', contig_len), pool))
        for lo, seq, qual, pos0, rev, rg in make():
            m = seq.shape[0]
            tab = np.full((m, 1), 9, dtype=np.uint8)
            text = lambda s: np.tile(np.frombuffer(s, dtype=np.uint8), (m, 1))
            flag = np.where(rev[:, None], text(b'80'), text(b'64'))                 # first of a pair whose mate is not given; 80: reverse
            line = np.concatenate([text(b'r'), digits(lo + np.arange(m), 8), tab, flag, tab, text(b'chr1'), tab, digits(pos0 + 1, pw),
                                   tab, text(b'60\t%dM\t*\t0\t0\t' % L), seq, tab, qual, text(b'\tRG:Z:g'), (48 + rg)[:, None].astype(np.uint8),
                                   np.full((m, 1), 10, dtype=np.uint8)], axis=1)
            sam.write(line.tobytes())
            nib = code[seq]
            body = np.concatenate([
                np.stack([np.zeros(m, np.int32), pos0.astype(np.int32)], axis=1).view(np.uint8),
                np.full((m, 1), 10, np.uint8), np.full((m, 1), 60, np.uint8),
                reg2bin(pos0, pos0 + L).astype(np.uint16)[:, None].view(np.uint8),
                np.full((m, 1), 1, np.uint16).view(np.uint8), np.where(rev, 80, 64).astype(np.uint16)[:, None].view(np.uint8),
                np.stack([np.full(m, L, np.int32), np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.zeros(m, np.int32)], axis=1).view(np.uint8),
                text(b'r'), digits(lo + np.arange(m), 8), np.zeros((m, 1), np.uint8),
                np.full((m, 1), L << 4, np.uint32).view(np.uint8), (nib[:, 0::2] << 4) | nib[:, 1::2], qual - 33,
                text(b'RGZg'), (48 + rg)[:, None].astype(np.uint8), np.zeros((m, 1), np.uint8)], axis=1)
            rec = np.concatenate([np.full((m, 1), body.shape[1], np.int32).view(np.uint8), body], axis=1)
            bam.write(bgzf(rec.tobytes(), pool))
        bam.write(bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000'))     # BGZF's empty last block


STAGES = re.compile(r'^kbbq stages: (.*?)  \(sum ', re.M)


def run(argv, tree, extra_env=None):
    """One command as a process: (wall seconds, {stage: seconds} from KBBQ_TIMING=1, stderr)."""
    env = dict(os.environ, PYTHONPATH=os.path.join(tree, 'kbbq-py_amd'), KBBQ_TIMING='1', **(extra_env or {}))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS'):
        env.pop(var, None)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, '-m', 'kbbq.main'] + argv, env=env, capture_output=True, timeout=1200)
    wall = time.perf_counter() - t0
    err = r.stderr.decode('utf-8', 'replace')
    if r.returncode:
        sys.exit('%s failed (%d):\n%s' % (' '.join(argv), r.returncode, err[-3000:]))
    stages = {}
    for line in STAGES.findall(err):
        for item in line.split('  '):
            name, value = item.rsplit(' ', 1)
            stages[name] = stages.get(name, 0.0) + float(value.rstrip('s'))
    return wall, stages, err


def planes_of(path, out):
    """recalibrate.LAST_RUN['aligned'] of the one run on `path`, from a process that calls the function."""
    code = ('import json, sys\nfrom kbbq import recalibrate\nrecalibrate.recalibrate_bam(sys.argv[1], kmers=dict(k=%d), output=sys.argv[2])\n'
            'sys.stderr.write("LAST_RUN " + json.dumps(recalibrate.LAST_RUN["aligned"]) + "\\n")\n' % args.k)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
    r = subprocess.run([sys.executable, '-c', code, path, out], env=env, capture_output=True, timeout=1200)
    if r.returncode:
        sys.exit('recalibrate_bam failed:\n%s' % r.stderr.decode('utf-8', 'replace')[-3000:])
    return json.loads(re.search(r'^LAST_RUN (.*)$', r.stderr.decode(), re.M).group(1))


def median_stages(runs):
    names = []
    for s in runs:
        names += [k for k in s if k not in names]
    return {k: round(float(np.median([s.get(k, 0.0) for s in runs])), 4) for k in names}


def main():
    tmp = args.dir or tempfile.mkdtemp(prefix='kbbq-time-bam-')
    os.makedirs(tmp, exist_ok=True)
    sam, bam = os.path.join(tmp, 'aln.sam'), os.path.join(tmp, 'aln.bam')
    t0 = time.perf_counter()
    write_set(sam, bam)
    two_tree = args.two_commands_tree or ROOT
    pitch = (L + 15) // 16 * 16
    res = dict(reads=n, len=L, k=args.k, genome=G, err=args.err, reps=args.reps, write_set_s=round(time.perf_counter() - t0, 1),
               two_commands_from='this tree' if two_tree == ROOT else 'the tree given', files={})
    for kind, path in (('sam', sam), ('bam', bam)):
        grp1, out1, grp2, out2 = (os.path.join(tmp, x) for x in ('one.grp', 'one.sam', 'two.grp', 'two.sam'))

        def one():
            if os.path.exists(grp1):
                os.unlink(grp1)
            return run(['recalibrate', '-b', path, '--kmers', '-k', str(args.k), '-g', grp1, '-o', out1], ROOT)

        def two():
            a = run(['bqsr', '-b', path, '--kmers', '-k', str(args.k), '-g', grp2], two_tree)
            b = run(['applybqsr', '-b', path, '-g', grp2, '-o', out2], two_tree)
            return a, b
        one(); two()                                                    # the warm-up: page cache, code objects on disk
        walls1, stages1, walls2, stages2a, stages2b, walls2a, walls2b = [], [], [], [], [], [], []
        for _ in range(args.reps):
            w, s, err = one()
            walls1.append(w); stages1.append(s)
            (wa, sa, _), (wb, sb, _) = two()
            walls2.append(wa + wb); walls2a.append(wa); walls2b.append(wb); stages2a.append(sa); stages2b.append(sb)
        same = open(out1, 'rb').read() == open(out2, 'rb').read() and open(grp1, 'rb').read() == open(grp2, 'rb').read()
        res['files'][kind] = dict(
            bytes=os.path.getsize(path), same_bytes=same,
            one_command_s=round(float(np.median(walls1)), 3), one_command_all=[round(w, 3) for w in walls1],
            two_commands_s=round(float(np.median(walls2)), 3), two_commands_all=[round(w, 3) for w in walls2],
            bqsr_s=round(float(np.median(walls2a)), 3), applybqsr_s=round(float(np.median(walls2b)), 3),
            saved_s=round(float(np.median(walls2)) - float(np.median(walls1)), 3),
            stages_one=median_stages(stages1), stages_bqsr=median_stages(stages2a), stages_applybqsr=median_stages(stages2b),
            aligned=planes_of(path, out1), two_commands_plane_bytes=4 * n * pitch,
            line=[ln for ln in err.split('\n') if ln.startswith('kbbq recalibrate:')])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
