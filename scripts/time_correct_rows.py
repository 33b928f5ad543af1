#!/usr/bin/env python3
"""Timing of `kbbq recalibrate -c` ("One file").

--kernels: km_count / km_correct on character planes against the 4-bit forms, on the same device-resident synthetic reads
(scripts/time_correct.py's: `--reads` x `--len` bases from both strands of a random genome at `--depth` x, `--err` uniform
substitutions) and against the same table.  The forms: `chars` (one read per row, pitch 160 for 150 bases), `reads_nib` (the
same rows as 4-bit planes) and `pairs_nib` (two reads to a row, 4-bit planes: what the file path keeps for reads of one
length).  HIP events, one warm-up, the median and the range of `--reps`; a fresh table for every count.  The run fails unless
the three tables hold the same histogram and the corrected planes are the same characters.  With --skip every repetition also
times kmer.correct_batch(skip_unresolved=True) on the same table (kbbq_kmer_correct_rows_skip_dev: the tally plane of `recalibrate
-c --skip-unresolved` beside the corrected plane; "ms_correct_skip", "skipped_bases"); the run fails unless the forms skip the
same number of bases.

--command FILE: writes `--reads` single-end reads to FILE (unless it exists), then wall time and KBBQ_TIMING stage lines of
`kbbq recalibrate -c FILE -o out` against `kbbq correct -f FILE -o cor` followed by `kbbq recalibrate -f FILE cor -o out`, each
`--reps` times after one warm-up run, and whether the two outputs are the same bytes.

Prints one JSON line per leg."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=16_000_000)
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--depth', type=float, default=30.0)
ap.add_argument('--err', type=float, default=0.01)
ap.add_argument('-k', type=int, default=31)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--kernels', action='store_true')
ap.add_argument('--skip', action='store_true', help='with --kernels: also time the correction that writes the tally plane')
ap.add_argument('--command', metavar='FILE', default=None)
args = ap.parse_args()

import numpy as np
import torch

n, L, k = args.reads, args.len, args.k
pitch = (L + 15) // 16 * 16
G = max(int(n * L / args.depth), 10 * L)


def slices(step=1 << 22):
    """(lo, uint8 [m, L] of ACGT characters on the device) over all reads."""
    g = torch.Generator(device='cuda').manual_seed(5)
    genome = torch.randint(0, 4, (G,), device='cuda', generator=g, dtype=torch.uint8)
    acgt = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device='cuda')
    col = torch.arange(L, device='cuda')
    for lo in range(0, n, step):
        m = min(step, n - lo)
        start = torch.randint(0, G - L + 1, (m, 1), device='cuda', generator=g)
        b = genome[start + col]
        rev = torch.rand((m, 1), device='cuda', generator=g) < 0.5
        b = torch.where(rev, (3 - b).flip(1), b)
        err = torch.rand((m, L), device='cuda', generator=g) < args.err
        b = torch.where(err, (b + torch.randint(1, 4, (m, L), device='cuda', generator=g, dtype=torch.uint8)) % 4, b)
        yield lo, acgt[b.long()]


def spread(v):
    return {'median': round(float(np.median(v)), 3), 'min': round(float(min(v)), 3), 'max': round(float(max(v)), 3)}


def kernels():
    from kbbq import _device as dev
    from kbbq import _native as N
    from kbbq import kmer
    plain = dev.ReadBatch(n, pitch, with_corrected=False)
    plain.seq.fill_(ord('N'))
    plain.qual.zero_()
    for lo, chars in slices():
        plain.seq[lo:lo + chars.shape[0], :L] = chars
        plain.qual[lo:lo + chars.shape[0], :L] = 33 + 30
    plain.meta.fill_(L)
    forms = {'chars': plain, 'reads_nib': dev.lay_out(plain, 1, pairs=False), 'pairs_nib': dev.lay_out(plain, 1, pairs=True)}
    assert [f.layout_key() for f in forms.values()] == ['reads', 'reads_nib', 'pairs_nib']
    windows = n * max(L - k + 1, 0)
    slots = 1 << int(np.ceil(np.log2((G + windows * args.err * k) * 2)))
    res = {'leg': 'kernels', 'reads': n, 'len': L, 'k': k, 'slots': slots, 'reps': args.reps}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    hists, planes = {}, {}
    for name, batch in forms.items():
        count, correct, skipping = [], [], []
        for rep in range(args.reps + 1):
            table = kmer.KmerTable(k, slots)
            torch.cuda.synchronize()
            c = timed(lambda: kmer.count_batch(batch, table=table))
            hist = kmer.kmer_histogram(table)
            t = kmer.solid_threshold(hist)
            x = timed(lambda: kmer.correct_batch(table, batch, t))
            if args.skip:
                got = []
                s = timed(lambda: got.append(kmer.correct_batch(table, batch, t, skip_unresolved=True)))
                skipped = int(got[0][1].sum(dtype=torch.int64).item())
                batch.tally_qual = None
            table.close()
            if rep:
                count.append(c)
                correct.append(x)
                if args.skip:
                    skipping.append(s)
        hists[name] = hist
        planes[name] = batch.chars('cseq')
        res[name] = {'pitch': batch.pitch, 'seq_bytes': int(batch.seq.numel()), 'ms_count': spread(count), 'ms_correct': spread(correct),
                     'min_count': t}
        if args.skip:
            res[name].update(ms_correct_skip=spread(skipping), skipped_bases=skipped, tally_plane_bytes=int(batch.qual.numel()))
    ref = planes['chars'][:, :L]
    pairs = planes.pop('pairs_nib')
    assert all(np.array_equal(h, hists['chars']) for h in hists.values()), 'the forms counted different tables'
    assert torch.equal(planes['reads_nib'][:, :L], ref), 'reads_nib corrected differently'
    assert torch.equal(pairs[:, :L], ref[0::2]) and torch.equal(pairs[:n // 2, L + 1:2 * L + 1], ref[1::2]), 'pairs_nib corrected differently'
    if args.skip:
        assert len({res[name]['skipped_bases'] for name in forms}) == 1, 'the forms skipped different numbers of bases'
    res['changed_bases'] = int((ref != plain.seq[:, :L]).sum().item())
    print(json.dumps(res), flush=True)


def write_fastq(path):
    digits = len(str(n - 1))
    rec = 1 + 1 + digits + 1 + L + 3 + L + 1
    q = np.random.default_rng(2).integers(2, 41, size=(1 << 16, L)).astype(np.uint8) + 33
    with open(path, 'wb') as fh:
        for lo, chars in slices(1 << 20):
            m = chars.shape[0]
            out = np.empty((m, rec), dtype=np.uint8)
            out[:, 0], out[:, 1] = ord('@'), ord('r')
            ids = np.arange(lo, lo + m)
            for d in range(digits):
                out[:, 2 + d] = 48 + (ids // 10 ** (digits - 1 - d)) % 10
            at = 2 + digits
            out[:, at] = 10
            out[:, at + 1:at + 1 + L] = chars.cpu().numpy()
            out[:, at + 1 + L:at + 4 + L] = np.frombuffer(b'\n+\n', dtype=np.uint8)
            out[:, at + 4 + L:at + 4 + 2 * L] = q[ids % q.shape[0]]
            out[:, -1] = 10
            fh.write(out.tobytes())


def run(*argv):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'), KBBQ_TIMING='1')
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, env=env)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()
    return wall, r.stderr.decode()


def command(path):
    if not os.path.exists(path):
        write_fastq(path)
        torch.cuda.empty_cache()
    one, two, cor = path + '.one.out', path + '.two.out', path + '.cor'
    res = {'leg': 'command', 'reads': n, 'len': L, 'file_bytes': os.path.getsize(path), 'reps': args.reps}
    walls = {'one': [], 'correct': [], 'recalibrate_f': []}
    for rep in range(args.reps + 1):
        w1, e1 = run('recalibrate', '-c', path, '-o', one)
        wc, ec = run('correct', '-f', path, '-o', cor)
        wr, er = run('recalibrate', '-f', path, cor, '-o', two)
        if rep:
            walls['one'].append(w1)
            walls['correct'].append(wc)
            walls['recalibrate_f'].append(wr)
    res.update({'s_' + key: spread(v) for key, v in walls.items()})
    res['s_two'] = spread([a + b for a, b in zip(walls['correct'], walls['recalibrate_f'])])
    res['ratio_two_over_one'] = round(res['s_two']['median'] / res['s_one']['median'], 3)
    res['stages'] = {'one': e1.splitlines(), 'correct': ec.splitlines(), 'recalibrate_f': er.splitlines()}
    with open(one, 'rb') as a, open(two, 'rb') as b:
        same = True
        while same:
            x, y = a.read(1 << 24), b.read(1 << 24)
            same = x == y
            if not x:
                break
    res['same_bytes'] = bool(same)
    for p in (one, two, cor):
        os.unlink(p)
    print(json.dumps(res), flush=True)


if args.kernels:
    kernels()
if args.command:
    command(args.command)
