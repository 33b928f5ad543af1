#!/usr/bin/env python3
"""Timing of `kbbq benchmark --kmers`.

1. The joint tally kernel (kbbq_flag_confusion_dev: quality, truth flags and k-mer flags, 3 B/base) beside K5 in its one-plane
   form (kbbq_count_q_dev with d_skip == NULL: quality and flags, 2 B/base) on the same synthetic rows, HIP-event time, the two
   alternating.  By bytes the new kernel should cost about 1.5x K5.
2. The stage times of the command's Python path (kbbq.benchmark.benchmark with kmers=...) on a truth set generated here (SAM text,
   FASTA, VCF): reader, reference and sites, upload + K4, qualities, the k-mer stages, the joint tally, the table.

With --passes P the command runs with `--passes P` (the k-mer flags of P passes of the rule).

No oracle and no file of the repository's is read; everything is generated from --seed."""
import argparse, contextlib, io, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=4_000_000, help='rows of the kernel timing')
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--records', type=int, default=200_000, help='alignments of the generated truth set (0: skip the stage times)')
ap.add_argument('--genome', type=int, default=1_000_000, help='bases of the generated reference')
ap.add_argument('-k', '--kmer', type=int, default=31)
ap.add_argument('--seed', type=int, default=1)
ap.add_argument('--passes', type=int, default=None, help='run the command with --passes P (1..8)')
a = ap.parse_args()
import numpy as np, torch
from kbbq import _device as dev, _native as N

# ---------------------------------------------------------------- 1. the kernel beside K5
n, L = a.reads, a.len
pitch = (L + 15) // 16 * 16
gen = torch.Generator(device='cuda'); gen.manual_seed(a.seed)
qual = torch.randint(2, 42, (n, pitch), dtype=torch.uint8, device='cuda', generator=gen)
r = torch.rand((n, pitch), device='cuda', generator=gen)
truth = (r < 0.01).to(torch.uint8) | ((r > 0.97).to(torch.uint8) << 1)                  # 1 % errors, 3 % skipped sites
r = torch.rand((n, pitch), device='cuda', generator=gen)
kflags = (r < 0.015).to(torch.uint8) | ((r > 0.9).to(torch.uint8) << 1)                 # 1.5 % flagged, 10 % unresolved
del r
lens = torch.full((n,), L, dtype=torch.int32, device='cuda')
c512 = torch.zeros(512, dtype=torch.int64, device='cuda')
c1536 = torch.zeros(1536, dtype=torch.int64, device='cuda')
ctx, lib = dev.context(), N.load()
def k5():
    N.check(lib.kbbq_count_q_dev(ctx.handle, N.ptr(qual), N.ptr(truth), None, N.ptr(lens), n, pitch, 0, N.ptr(c512)))
def k5j():
    N.check(lib.kbbq_flag_confusion_dev(ctx.handle, N.ptr(qual), N.ptr(truth), N.ptr(kflags), N.ptr(lens), n, pitch, 0, N.ptr(c1536)))
def event_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)
for f in (k5, k5j, k5, k5j):
    f()
torch.cuda.synchronize()
ms = {'k5': [], 'k5j': []}
for _ in range(a.reps):                                       # the two alternate: what shares the machine shares both
    ms['k5'].append(event_ms(k5)); ms['k5j'].append(event_ms(k5j))
ctx.status()
joint = c1536.cpu().numpy().reshape(256, 2, 3) // (a.reps + 2)
both = c512.cpu().numpy() // (a.reps + 2)
assert np.array_equal(joint.sum(axis=(1, 2)), both[:256]) and np.array_equal(joint[:, 1].sum(axis=1), both[256:]), 'the two kernels disagree'
med = {k: float(np.median(v)) for k, v in ms.items()}
for name, key, bpb in (('K5 count_q <- flags plane', 'k5', 2), ('joint tally (kbbq_flag_confusion_dev)', 'k5j', 3)):
    print('%s: median %.3f ms, min %.3f, max %.3f of %d for %d reads x %d = %.0f GB/s algorithmic (%d B/base)'
          % (name, med[key], min(ms[key]), max(ms[key]), a.reps, n, L, bpb * n * L / med[key] / 1e6, bpb), flush=True)
print('joint tally / K5: %.2f x (by bytes: 1.50)' % (med['k5j'] / med['k5']), flush=True)
del qual, truth, kflags
torch.cuda.empty_cache()

# ---------------------------------------------------------------- 2. the command's stages on a generated truth set
if a.records:
    from kbbq import benchmark as bm, kmer
    rng = np.random.default_rng(a.seed)
    G, m = a.genome, a.records
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    genome = letters[rng.integers(0, 4, G)]
    tmp = tempfile.mkdtemp(prefix='kbbq_time_benchmark_kmers_')
    fa, vcf, sam = (os.path.join(tmp, x) for x in ('ref.fa', 'sites.vcf', 'truth.sam'))
    with open(fa, 'wb') as fh:
        fh.write(b'>chr1\n')
        text = genome.tobytes()
        fh.write(b'\n'.join(text[i:i + 60] for i in range(0, G, 60)) + b'\n')
    sites = np.sort(rng.choice(G - 1, size=G // 1000, replace=False))
    with open(vcf, 'w') as fh:
        fh.write('##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
        fh.writelines('chr1\t%d\t.\t%s\tA\t30\t.\t.\n' % (p + 1, chr(genome[p])) for p in sites)
    start = rng.integers(0, G - L, m)
    seq = genome[start[:, None] + np.arange(L)[None, :]].copy()
    sub = rng.random((m, L)) < 0.01
    seq[sub] = letters[rng.integers(0, 4, int(sub.sum()))]
    q = (rng.integers(2, 42, (m, L)) + 33).astype(np.uint8)
    with open(sam, 'w') as fh:
        fh.write('@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:%d\n' % G)
        fh.writelines('r%d\t0\tchr1\t%d\t60\t%dM\t*\t0\t0\t%s\t%s\n' % (i, start[i] + 1, L, seq[i].tobytes().decode(), q[i].tobytes().decode())
                      for i in range(m))
    stages = []
    def timed(mod, name, label=None):
        f = getattr(mod, name)
        def g(*args, **kw):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = f(*args, **kw)
            torch.cuda.synchronize(); stages.append((label or name, time.perf_counter() - t0))
            return out
        setattr(mod, name, g)
    timed(bm.aln.AlignmentFile, '__init__', 'open the SAM file (the reader parses it)')
    timed(bm, '_kmer_benchmark_inputs', 'argument checks')
    timed(bm, 'get_ref_dict', 'FASTA'); timed(bm, 'get_var_sites', 'VCF'); timed(bm, 'get_full_skips', 'skip mask')
    timed(bm, '_Genome', 'reference upload')
    timed(bm, '_flag_batch', 'SEQ plane + CIGARs + upload + K4'); timed(bm, '_qual_chars_dev', 'quality plane + upload + check')
    timed(kmer, 'count_kmers', 'k-mer count'); timed(kmer, 'kmer_histogram', 'k-mer histogram'); timed(kmer, 'flag_errors', 'k-mer flags')
    timed(bm, 'kmer_confusion', 'joint tally + download'); timed(bm, 'print_benchmark_kmers', 'table')
    def run():
        del stages[:]
        out, err = io.StringIO(), io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            bm.benchmark(sam, fa, vcf, label='timing', kmers=dict(k=a.kmer, **({} if a.passes is None else dict(passes=a.passes))))
        return time.perf_counter() - t0, err.getvalue().strip()
    run()                                                      # warm: code objects, the page cache
    total, line = run()
    print(line)
    print('kbbq benchmark --kmers -k %d%s on %d records x %d bases, genome %d: %.1f ms'
          % (a.kmer, '' if a.passes is None else ' --passes %d' % a.passes, m, L, G, total * 1e3))
    for name, dt in stages:
        print('  %-48s %8.2f ms  %4.1f %%' % (name, dt * 1e3, 100 * dt / total))
    print('  %-48s %8.2f ms  %4.1f %%' % ('(between the stages)', (total - sum(dt for _, dt in stages)) * 1e3,
                                          100 * (1 - sum(dt for _, dt in stages) / total)))
    shutil.rmtree(tmp)
