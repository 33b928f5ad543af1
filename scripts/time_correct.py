#!/usr/bin/env python3
"""Kernel timing (HIP events) of kbbq correct's three steps on device-resident synthetic reads: `--reads` x `--len` bases
sampled from both strands of a random genome sized for `--depth` x coverage, `--err` uniform substitutions.  Count
(kbbq_kmer_count_dev into a fresh table), histogram (kbbq_kmer_histogram_dev) and correct (kbbq_kmer_correct_dev) are each
timed once per repetition after a warm-up on the same table.  Prints one JSON line: ms per step, k-mer windows per second of
the count and of the correct step, the table's slots and bytes, its distinct k-mers, the threshold and the changed bases.
With `--prefilter` a second leg on the same reads follows under the key "prefilter": km_prefilter into a fresh filter, `seen`
released, a table sized from the filter's `admitted` (or `--prefilter-slots`), the filtered count, histogram and correct, each
timed the same way, with the filter's bytes and the device bytes in use at their peak (kbbq_dev_mem_info, planes excluded)
beside the plain leg's; the leg fails unless its threshold, hist[2:] and corrected plane equal the plain leg's.
With `--fix-n` every repetition also times kbbq_kmer_correct_ex_dev with KBBQ_KMER_FIX_N on the same table ("ms_correct_fix_n",
"fixed_n"); `--n-rate` sets that share of the bases to N before anything is counted.
With `--flags` every repetition also times kbbq_kmer_flag_dev (the decision as a flag plane, `kbbq bqsr --kmers`) on the same
table right after kbbq_kmer_correct_dev ("ms_flags", "flagged_bases"); the leg fails unless the plane is 1 exactly where the
corrected plane differs from the input.
With `--unresolved` (needs `--flags`) every repetition also times kbbq_kmer_flag_ex_dev with KBBQ_KMER_FLAG_UNRESOLVED right
after kbbq_kmer_flag_dev ("ms_flags_unresolved", "unresolved_bases"); the leg fails unless its plane with every 2 turned to 0
is kbbq_kmer_flag_dev's and its per-read counts add up to the plane's 1s and 2s.
With `--passes P` (2..8) every repetition also times, for p = 2 .. P, kbbq_kmer_correct_passes_dev with passes = p
("ms_correct_passes"[p]) and its yardstick, p successive kbbq_kmer_correct_dev launches that feed their plane back through
global memory against the same table ("ms_correct_repeated"[p]); the leg fails unless the two planes are equal.  With `--flags
--unresolved` also kbbq_kmer_flag_passes_dev with KBBQ_KMER_FLAG_UNRESOLVED ("ms_flags_unresolved_passes"[p], with the 1s and 2s
of its plane); the leg fails unless its 1s are where the corrected plane of p passes differs from the input.
With `--skip` every repetition also times kbbq_kmer_correct_rows_skip_dev (the corrected plane and, beside it, the tally plane of
`recalibrate -c --skip-unresolved`: the qualities with byte 0 at every unresolved base) on the same character rows and table
right after kbbq_kmer_correct_dev ("ms_correct_skip", "skipped_bases", "tally_plane_bytes"); the leg fails unless its corrected
plane is kbbq_kmer_correct_dev's and its tally plane is the quality plane with as many bytes zeroed as d_unresolved adds up to.
With `--partitions P` (2..64) a leg on the same reads follows under the key "partitions" (`kbbq correct --partitions P`,
kmer.count_partitioned spelt out call by call so that every step has its own events): per round kbbq_kmer_count_part_dev into
the per-partition table (`--partition-slots`, default kmer.partition_slots of the windows in the device budget), the histogram
and kbbq_kmer_select_*_dev of the pairs with count >= 2; then the merge of the kept pairs into the solid table and
kbbq_kmer_correct_dev against it.  "ms_count_rounds" has the median of every round, "ms_count" their sum, and "peak_bytes" the
device bytes at their peak, from the allocations made (kbbq_dev_mem_info for the library's, torch's count of live bytes for
the kept pairs; planes excluded; "peak_bytes_merge": while the solid table is built); the leg fails unless its
summed histogram, threshold and corrected plane equal the plain leg's.
With `--qual-model calibrated` the reads get qualities from {2, 12, 23, 37} with the shares of `--qual-shares` (per cent) and their
errors are drawn per base at the rate the quality states, 10^(-q/10), instead of `--err` everywhere, so that a quality gate has
something to gate.  The error-free plane is kept in either model, and every leg prints what its corrected plane did against it:
"errors" (bases inside the reads that differ from the truth and are no N), "errors_fixed" (those the leg set to the truth's
letter) and "false_changes" (bases the leg changed to a letter that is not the truth's).
With `--kmer-min-qual Q` (needs qualities: `--qual-model calibrated`, or `--skip`, whose qualities are uniform in 2..40) a leg on
the same reads follows under the key "gate" (`kbbq correct --kmer-min-qual Q`): kbbq_kmer_gate_rows_dev into a fresh plane
("ms_gate", and "gate_share_of_8TBs": its algorithmic bytes -- sequence read, qualities read, gated plane written -- per second
over the 8 TB/s of the spec), a table sized from the counted windows (or `--gate-slots`), kbbq_kmer_count_dev of the gated plane,
the histogram, the plane freed, kbbq_kmer_correct_dev of the reads as read; with the table's slots, bytes, load, distinct k-mers
and singletons, and the device bytes at their peak with the gated plane counted ("peak_bytes")."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
ap = argparse.ArgumentParser()
ap.add_argument('--reads', type=int, default=16_000_000)
ap.add_argument('--len', type=int, default=150)
ap.add_argument('--depth', type=float, default=30.0)
ap.add_argument('--err', type=float, default=0.01)
ap.add_argument('-k', type=int, default=31)
ap.add_argument('--slots', type=int, default=0, help='table slots (default: distinct k-mers expected at a load factor <= 0.5)')
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--prefilter', action='store_true', help='add the prefiltered leg')
ap.add_argument('--filter-bits', type=int, default=4)
ap.add_argument('--prefilter-slots', type=int, default=0, help='table slots of the prefiltered leg (default: from `admitted`)')
ap.add_argument('--fix-n', action='store_true', help='also time the correct step with the N rule (KBBQ_KMER_FIX_N)')
ap.add_argument('--flags', action='store_true', help='also time the flag form of the correct step (kbbq_kmer_flag_dev)')
ap.add_argument('--unresolved', action='store_true',
                help='with --flags: also time the flag form with unresolved bases as 2 (kbbq_kmer_flag_ex_dev)')
ap.add_argument('--passes', type=int, default=1,
                help='also time 2 .. P passes of the correct step in one launch (kbbq_kmer_correct_passes_dev) and as P launches')
ap.add_argument('--skip', action='store_true',
                help='also time the correct step that writes the tally plane beside the corrected one (kbbq_kmer_correct_rows_skip_dev)')
ap.add_argument('--partitions', type=int, default=1, help='add the leg that counts in this many rounds (kbbq correct --partitions)')
ap.add_argument('--partition-slots', type=int, default=0, help='slots of that leg\'s per-partition table')
ap.add_argument('--n-rate', type=float, default=0.0, help='share of the bases set to N')
ap.add_argument('--qual-model', choices=('uniform', 'calibrated'), default='uniform',
                help='calibrated: qualities from {2, 12, 23, 37} by --qual-shares, errors per base at 10^(-q/10) instead of --err')
ap.add_argument('--qual-shares', default='1,3,6,90', help='per cent of the bases at quality 2, 12, 23 and 37 (calibrated)')
ap.add_argument('--kmer-min-qual', type=int, default=0, help='add the leg that counts only k-mers of bases with quality >= Q')
ap.add_argument('--gate-slots', type=int, default=0, help='table slots of that leg (default: from the counted windows)')
args = ap.parse_args()
if args.unresolved and not args.flags:
    ap.error('--unresolved: only with --flags')
if not 1 <= args.passes <= 8:
    ap.error('--passes: 1..8')
if not 1 <= args.partitions <= 64:
    ap.error('--partitions: 1..64')
if not 0 <= args.kmer_min_qual <= 93:
    ap.error('--kmer-min-qual: 1..93')
if args.kmer_min_qual and args.qual_model != 'calibrated' and not args.skip:
    ap.error('--kmer-min-qual: needs qualities (--qual-model calibrated, or --skip)')
try:
    shares = [float(x) for x in args.qual_shares.split(',')]
    assert len(shares) == 4 and min(shares) >= 0 and abs(sum(shares) - 100) < 1e-6
except (ValueError, AssertionError):
    ap.error('--qual-shares: four numbers that add up to 100')

import numpy as np
import torch
from kbbq import _native as N
from kbbq import kmer

n, L, k = args.reads, args.len, args.k
pitch = (L + 15) // 16 * 16
G = max(int(n * L / args.depth), 10 * L)
g = torch.Generator(device='cuda').manual_seed(5)
genome = torch.randint(0, 4, (G,), device='cuda', generator=g, dtype=torch.uint8)
seq = torch.full((n, pitch), ord('N'), dtype=torch.uint8, device='cuda')
truth = torch.full((n, pitch), ord('N'), dtype=torch.uint8, device='cuda')      # the reads without their errors
calibrated = args.qual_model == 'calibrated'
qual = torch.zeros_like(seq) if calibrated else None                             # 0 in the padding
qvals = torch.tensor([2, 12, 23, 37], dtype=torch.uint8, device='cuda')
cuts = torch.tensor(np.cumsum(shares)[:3] / 100.0, dtype=torch.float32, device='cuda')
acgt = torch.tensor(list(b'ACGT'), dtype=torch.uint8, device='cuda')
col = torch.arange(L, device='cuda')
step = 1 << 22
for lo in range(0, n, step):                         # slices: the index tensors of all reads at once would not fit beside the planes
    m = min(step, n - lo)
    start = torch.randint(0, G - L + 1, (m, 1), device='cuda', generator=g)
    b = genome[start + col]
    rev = torch.rand((m, 1), device='cuda', generator=g) < 0.5
    b = torch.where(rev, (3 - b).flip(1), b)
    truth[lo:lo + m, :L] = acgt[b.long()]
    if calibrated:
        q = qvals[torch.bucketize(torch.rand((m, L), device='cuda', generator=g), cuts, right=True)]
        qual[lo:lo + m, :L] = q + 33
        err = torch.rand((m, L), device='cuda', generator=g) < torch.pow(10.0, -q.float() / 10.0)
        del q
    else:
        err = torch.rand((m, L), device='cuda', generator=g) < args.err
    b = torch.where(err, (b + torch.randint(1, 4, (m, L), device='cuda', generator=g, dtype=torch.uint8)) % 4, b)
    seq[lo:lo + m, :L] = acgt[b.long()]
    if args.n_rate > 0:
        seq[lo:lo + m, :L].masked_fill_(torch.rand((m, L), device='cuda', generator=g) < args.n_rate, ord('N'))
del genome
meta = torch.full((n,), L, dtype=torch.int32, device='cuda')
windows = n * max(L - k + 1, 0)
distinct = G + windows * args.err * k                  # the genome's k-mers and those an error makes
slots = args.slots or 1 << int(np.ceil(np.log2(distinct * 2)))
out = torch.empty_like(seq)
out2 = torch.empty_like(seq) if args.prefilter else None   # the prefiltered leg's plane, compared with the plain one
out_n = torch.empty_like(seq) if args.fix_n else None     # the plane of the correct step with the N rule
flags = torch.empty_like(seq) if args.flags else None     # the plane of the flag form
flags_u = torch.empty_like(seq) if args.unresolved else None      # ... with unresolved bases as 2
out_p = torch.empty_like(seq) if args.passes > 1 else None # the plane of several passes in one launch
ping = [torch.empty_like(seq), torch.empty_like(seq)] if args.passes > 1 else None        # ... and of as many launches
if args.skip:                                           # qualities 2..40 inside the reads, 0 in the padding; the tally plane
    if qual is None:
        qual = torch.zeros_like(seq)
        for lo in range(0, n, step):
            m = min(step, n - lo)
            qual[lo:lo + m, :L] = torch.randint(35, 74, (m, L), device='cuda', generator=g, dtype=torch.uint8)
    out_s, tally = torch.empty_like(seq), torch.empty_like(seq)
    s_unres = torch.empty((n,), dtype=torch.int32, device='cuda')
lib = N.load()


def in_use(ctx):
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    N.check(lib.kbbq_dev_mem_info(ctx.handle, ctypes.byref(free), ctypes.byref(total)))
    return total.value - free.value


def rep_base():
    """Device bytes in use before a repetition allocates anything: the planes, the runtime's own, torch's cached blocks."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return in_use(kmer._ctx())


def against_truth(plane):
    """What a corrected plane did, by the error-free plane: errors of the reads, those it fixed, and its changes to a letter that
    is not the truth's (sums of boolean planes: they have more than 2^31 elements)."""
    wrong = (seq != truth) & (seq != ord('N'))
    total = lambda x: int(x.sum(dtype=torch.int64).item())
    return {'errors': total(wrong), 'errors_fixed': total(wrong & (plane == truth)),
            'false_changes': total((plane != seq) & (plane != truth))}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


res = {'reads': n, 'len': L, 'k': k, 'genome': G, 'err': args.err, 'slots': slots,
       'table_bytes': int(lib.kbbq_kmer_table_bytes(slots))}
ms = {'count': [], 'histogram': [], 'correct': []}
if args.fix_n:
    ms['correct_fix_n'] = []
if args.skip:
    ms['correct_skip'] = []
if args.flags:
    ms['flags'] = []
if args.unresolved:
    ms['flags_unresolved'] = []
    n_err = torch.empty((n,), dtype=torch.int32, device='cuda')
    n_unres = torch.empty((n,), dtype=torch.int32, device='cuda')
PASSES = list(range(2, args.passes + 1))
ms_fused, ms_repeated, ms_flags_fused = {p: [] for p in PASSES}, {p: [] for p in PASSES}, {p: [] for p in PASSES}
changed_p, flagged_p, unresolved_p = {}, {}, {}
if PASSES and args.unresolved:
    p_err = torch.empty((n,), dtype=torch.int32, device='cuda')
    p_unres = torch.empty((n,), dtype=torch.int32, device='cuda')


def repeated(table, t, p):
    """p launches of the one-pass kernel, each on the plane of the one before; the last plane."""
    src = seq
    for i in range(p):
        dst = ping[i & 1]
        N.check(lib.kbbq_kmer_correct_dev(table.ctx.handle, table.handle, N.ptr(src), N.ptr(meta), n, pitch, t, N.ptr(dst), None))
        src = dst
    return src


dh = torch.zeros(257, dtype=torch.int64, device='cuda')
for rep in range(args.reps + 1):
    base = rep_base()
    table = kmer.KmerTable(k, slots)
    torch.cuda.synchronize()
    res['peak_bytes'] = in_use(table.ctx) - base
    c = timed(lambda: N.check(lib.kbbq_kmer_count_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch)))
    table.ctx.status()
    h = timed(lambda: N.check(lib.kbbq_kmer_histogram_dev(table.ctx.handle, table.handle, N.ptr(dh))))
    hist = dh.cpu().numpy()
    t = kmer.solid_threshold(hist)
    x = timed(lambda: N.check(lib.kbbq_kmer_correct_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                         N.ptr(out), None)))
    if args.skip:
        xs = timed(lambda: N.check(lib.kbbq_kmer_correct_rows_skip_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch,
                                                                       0, t, N.ptr(out_s), None, 0, 1, N.ptr(qual), N.ptr(tally),
                                                                       N.ptr(s_unres))))
    if args.fix_n:
        xn = timed(lambda: N.check(lib.kbbq_kmer_correct_ex_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                                N.ptr(out_n), None, N.KMER_FIX_N)))
    if args.flags:
        xf = timed(lambda: N.check(lib.kbbq_kmer_flag_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                          N.ptr(flags), None)))
    if args.unresolved:
        xu = timed(lambda: N.check(lib.kbbq_kmer_flag_ex_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                             N.ptr(flags_u), N.ptr(n_err), N.ptr(n_unres),
                                                             N.KMER_FLAG_UNRESOLVED)))
    for p in PASSES:
        xp = timed(lambda: N.check(lib.kbbq_kmer_correct_passes_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch,
                                                                    t, N.ptr(out_p), None, 0, p)))
        xr = timed(lambda: repeated(table, t, p))
        assert torch.equal(out_p, ping[(p - 1) & 1]), '%d passes in one launch are not %d launches' % (p, p)
        changed_p[p] = int((out_p != seq).sum().item())
        if args.unresolved:
            xq = timed(lambda: N.check(lib.kbbq_kmer_flag_passes_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch,
                                                                     t, N.ptr(flags_u), N.ptr(p_err), N.ptr(p_unres),
                                                                     N.KMER_FLAG_UNRESOLVED, p)))
            assert torch.equal(flags_u == 1, out_p != seq), 'the flag form of %d passes decided differently from the correction' % p
            flagged_p[p] = int(p_err.sum(dtype=torch.int64).item())
            unresolved_p[p] = int(p_unres.sum(dtype=torch.int64).item())
            assert unresolved_p[p] == int((flags_u == 2).sum(dtype=torch.int64).item()), 'd_unresolved does not add up to the 2s'
        if rep:
            ms_fused[p].append(xp); ms_repeated[p].append(xr)
            if args.unresolved:
                ms_flags_fused[p].append(xq)
    if PASSES and args.unresolved:                     # the plane the checks below read is the one-pass one
        N.check(lib.kbbq_kmer_flag_ex_dev(table.ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t, N.ptr(flags_u),
                                          N.ptr(n_err), N.ptr(n_unres), N.KMER_FLAG_UNRESOLVED))
        torch.cuda.synchronize()
    table.close()
    if rep:                                            # the first round is the warm-up
        ms['count'].append(c); ms['histogram'].append(h); ms['correct'].append(x)
        if args.flags:
            ms['flags'].append(xf)
        if args.unresolved:
            ms['flags_unresolved'].append(xu)
        if args.fix_n:
            ms['correct_fix_n'].append(xn)
        if args.skip:
            ms['correct_skip'].append(xs)
res.update({'ms_' + key: round(float(np.median(v)), 3) for key, v in ms.items()})
res['count_kmers_per_s'] = windows / (res['ms_count'] * 1e-3)
res['correct_kmers_per_s'] = windows / (res['ms_correct'] * 1e-3)
res['distinct'] = int(hist.sum())
res['load_factor'] = round(res['distinct'] / slots, 3)
res['min_count'] = t
res['changed_bases'] = int((out != seq).sum().item())
res['ms_correct_all'] = [round(v, 3) for v in ms['correct']]
res['singletons'] = int(hist[1])
res['qual_model'] = args.qual_model
res.update(against_truth(out))
if args.kmer_min_qual:
    from kbbq import _device as dev
    Q = args.kmer_min_qual
    plain_out, plain_hist, plain_t = out, hist, t
    out_g = ping[0] if ping else torch.empty_like(seq)
    ms = {'gate': [], 'count': [], 'histogram': [], 'correct': []}
    for rep in range(args.reps + 1):
        base = rep_base()
        ctx = kmer._ctx()
        gated = torch.empty_like(seq)
        word = torch.zeros(1, dtype=torch.int64, device='cuda')
        gt = timed(lambda: N.check(lib.kbbq_kmer_gate_rows_dev(ctx.handle, N.ptr(seq), N.ptr(qual), N.ptr(meta), n, pitch, 0, k, Q + 33,
                                                               N.ptr(gated), N.ptr(word))))
        ctx.status()
        counted = int(word.item())
        gslots = args.gate_slots or kmer.default_slots(counted, dev.device_budget())
        table = kmer.KmerTable(k, gslots)
        torch.cuda.synchronize()
        peak = in_use(ctx) - base                      # the gated plane and the table: the planes of the reads are in `base`
        c = timed(lambda: N.check(lib.kbbq_kmer_count_dev(ctx.handle, table.handle, N.ptr(gated), N.ptr(meta), n, pitch)))
        ctx.status()
        h = timed(lambda: N.check(lib.kbbq_kmer_histogram_dev(ctx.handle, table.handle, N.ptr(dh))))
        hist = dh.cpu().numpy()
        t = kmer.solid_threshold(hist)
        del gated                                      # the count is over: the correction reads the reads as read
        x = timed(lambda: N.check(lib.kbbq_kmer_correct_dev(ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                             N.ptr(out_g), None)))
        table.close()
        if rep:
            for key, v in zip(ms, (gt, c, h, x)):
                ms[key].append(v)
    leg = {'kmer_min_qual': Q, 'counted_windows': counted, 'windows': windows, 'slots': gslots,
           'table_bytes': int(lib.kbbq_kmer_table_bytes(gslots)), 'gated_plane_bytes': n * pitch, 'peak_bytes': peak}
    leg.update({'ms_' + key: round(float(np.median(v)), 3) for key, v in ms.items()})
    leg['ms_gate_all'] = [round(v, 3) for v in ms['gate']]
    leg['ms_correct_all'] = [round(v, 3) for v in ms['correct']]
    leg['gate_bytes'] = 3 * n * pitch                  # character rows: sequence read, qualities read, gated plane written
    leg['gate_share_of_8TBs'] = round(leg['gate_bytes'] / (leg['ms_gate'] * 1e-3) / 8e12, 3)
    leg.update(distinct=int(hist.sum()), singletons=int(hist[1]), load_factor=round(int(hist.sum()) / gslots, 3), min_count=t,
               changed_bases=int((out_g != seq).sum().item()), differs_from_plain=int((out_g != plain_out).sum().item()),
               count_kmers_per_s=counted / (leg['ms_count'] * 1e-3), correct_kmers_per_s=windows / (leg['ms_correct'] * 1e-3))
    leg.update(against_truth(out_g))
    res['gate'] = leg
    hist, t = plain_hist, plain_t
    del out_g
if args.fix_n:
    res['n_rate'] = args.n_rate
    res['n_bases'] = int((seq[:, :L] == ord('N')).sum().item())
    res['fixed_n'] = int(((out_n != seq) & (seq == ord('N'))).sum().item())
    res['ms_correct_fix_n_all'] = [round(v, 3) for v in ms['correct_fix_n']]
    # (no boolean indexing: the planes have more than 2^31 elements)
    assert torch.equal(torch.where(seq != ord('N'), out_n, out), out), 'the N rule changed a base that is no N'
if args.skip:
    res['ms_correct_skip_all'] = [round(v, 3) for v in ms['correct_skip']]
    res['skipped_bases'] = int(s_unres.sum(dtype=torch.int64).item())
    res['tally_plane_bytes'] = n * pitch
    assert torch.equal(out_s, out), 'the corrected plane beside the tally plane is not kbbq_kmer_correct_dev\'s'
    assert torch.equal(torch.where(tally == 0, torch.zeros_like(qual), qual), tally), 'the tally plane changed a byte it did not zero'
    assert int(((tally == 0) & (qual != 0)).sum(dtype=torch.int64).item()) == res['skipped_bases'], 'd_unresolved does not add up to the zeros'
if args.flags:
    res['ms_flags_all'] = [round(v, 3) for v in ms['flags']]
    res['flags_kmers_per_s'] = windows / (res['ms_flags'] * 1e-3)
    res['flagged_bases'] = int(flags.sum(dtype=torch.int64).item())
    assert torch.equal(flags, (out != seq).to(torch.uint8)), 'the flag form decided differently from the correction'
if args.unresolved:
    res['ms_flags_unresolved_all'] = [round(v, 3) for v in ms['flags_unresolved']]
    res['unresolved_bases'] = int((flags_u == 2).sum(dtype=torch.int64).item())
    assert torch.equal(torch.where(flags_u == 2, torch.zeros_like(flags_u), flags_u), flags), 'the option changed a byte that is no 2'
    assert int(n_err.sum(dtype=torch.int64).item()) == res['flagged_bases'], 'd_changed does not add up to the 1s'
    assert int(n_unres.sum(dtype=torch.int64).item()) == res['unresolved_bases'], 'd_unresolved does not add up to the 2s'
if PASSES:
    spread = lambda v: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)]       # median, fastest, slowest
    res['ms_correct_passes'] = {str(p): spread(ms_fused[p]) for p in PASSES}
    res['ms_correct_repeated'] = {str(p): spread(ms_repeated[p]) for p in PASSES}
    res['changed_bases_passes'] = {str(p): changed_p[p] for p in PASSES}
    if args.unresolved:
        res['ms_flags_unresolved_passes'] = {str(p): spread(ms_flags_fused[p]) for p in PASSES}
        res['flagged_bases_passes'] = {str(p): flagged_p[p] for p in PASSES}
        res['unresolved_bases_passes'] = {str(p): unresolved_p[p] for p in PASSES}
if args.prefilter:
    from kbbq import _device as dev
    plain_out, plain_hist, plain_t = out, hist, t
    out = out2
    words = kmer.filter_words(windows, args.filter_bits)
    ms = {'prefilter': [], 'count_filtered': [], 'histogram': [], 'correct': []}
    leg = {'filter_bits': args.filter_bits, 'filter_words': words, 'filter_bytes': int(lib.kbbq_kmer_filter_bytes(words))}
    for rep in range(args.reps + 1):
        base = rep_base()
        filt = kmer.KmerFilter(words)
        torch.cuda.synchronize()
        peak = in_use(filt.ctx) - base
        ctx = filt.ctx
        f = timed(lambda: N.check(lib.kbbq_kmer_prefilter_dev(ctx.handle, filt.handle, k, N.ptr(seq), N.ptr(meta), n, pitch)))
        admitted = filt.admitted
        filt.release_seen()
        pslots = args.prefilter_slots or kmer.default_slots(admitted, dev.device_budget())
        table = kmer.KmerTable(k, pslots)
        torch.cuda.synchronize()
        peak = max(peak, in_use(ctx) - base)
        c = timed(lambda: N.check(lib.kbbq_kmer_count_filtered_dev(ctx.handle, table.handle, filt.handle, N.ptr(seq), N.ptr(meta),
                                                                   n, pitch)))
        ctx.status()
        filt.close()
        h = timed(lambda: N.check(lib.kbbq_kmer_histogram_dev(ctx.handle, table.handle, N.ptr(dh))))
        hist = dh.cpu().numpy()
        t = kmer.solid_threshold(hist)
        x = timed(lambda: N.check(lib.kbbq_kmer_correct_dev(ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                             N.ptr(out), None)))
        table.close()
        if rep:
            for key, v in zip(ms, (f, c, h, x)):
                ms[key].append(v)
    leg.update({'ms_' + key: round(float(np.median(v)), 3) for key, v in ms.items()})
    leg.update(slots=pslots, table_bytes=int(lib.kbbq_kmer_table_bytes(pslots)), admitted=admitted, peak_bytes=peak,
               entries=int(hist.sum()), admitted_singletons=int(hist[1]), load_factor=round(int(hist.sum()) / pslots, 3),
               min_count=t, prefilter_kmers_per_s=windows / (leg['ms_prefilter'] * 1e-3),
               count_filtered_kmers_per_s=windows / (leg['ms_count_filtered'] * 1e-3))
    assert t == plain_t and np.array_equal(hist[2:], plain_hist[2:]), 'the prefiltered leg found another histogram'
    assert torch.equal(out, plain_out), 'the prefiltered leg corrected differently'
    leg['singletons'] = int(plain_hist[1])
    res['prefilter'] = leg
if args.partitions > 1:
    from kbbq import _device as dev
    P = args.partitions
    plain_out = out2 if args.prefilter else out        # (the prefiltered leg checked out2 against the plain plane)
    plain_hist, plain_t = (plain_hist, plain_t) if args.prefilter else (hist, t)
    out = ping[0] if ping else torch.empty_like(seq)
    budget = dev.device_budget()
    qslots = args.partition_slots or kmer.partition_slots(windows, P, budget)
    ms = {'count_rounds': [[] for _ in range(P)], 'histogram': [], 'select': [], 'merge': [], 'correct': []}
    def held(ctx):
        """Device bytes of the allocations made: the library's (the device's bytes in use less what torch has reserved) and the
        live tensors (the kept pairs come from torch, which may serve them from segments it reserved long before)."""
        return in_use(ctx) - torch.cuda.memory_reserved() + torch.cuda.memory_allocated()

    for rep in range(args.reps + 1):
        rep_base()
        base = held(kmer._ctx())
        table = kmer.KmerTable(k, qslots)
        ctx = table.ctx
        hsum, kept = np.zeros(257, dtype=np.int64), []
        cs, hs, ss = [], 0.0, 0.0
        peak = 0
        for p in range(P):
            if p:
                table.clear()
            cs.append(timed(lambda: N.check(lib.kbbq_kmer_count_part_dev(ctx.handle, table.handle, N.ptr(seq), N.ptr(meta), n, pitch,
                                                                          P, p))))
            ctx.status()
            hs += timed(lambda: N.check(lib.kbbq_kmer_histogram_dev(ctx.handle, table.handle, N.ptr(dh))))
            hsum += dh.cpu().numpy()
            got = []
            ss += timed(lambda: got.append(kmer.select(table, 1, 2)))
            kept.append(got[0][:2])
            peak = max(peak, held(ctx) - base)
        table.close()
        t = kmer.solid_threshold(hsum)
        npairs = sum(int(a.shape[0]) for a, _ in kept)
        solid = kmer.KmerTable(k, kmer.default_slots(npairs, budget))
        torch.cuda.synchronize()
        peak_solid = held(ctx) - base
        peak = max(peak, peak_solid)
        m = timed(lambda: [kmer.merge(solid, a, b) for a, b in kept])
        del kept, got
        x = timed(lambda: N.check(lib.kbbq_kmer_correct_dev(ctx.handle, solid.handle, N.ptr(seq), N.ptr(meta), n, pitch, t,
                                                             N.ptr(out), None)))
        solid_slots = solid.slots
        solid.close()
        if rep:
            for p in range(P):
                ms['count_rounds'][p].append(cs[p])
            ms['histogram'].append(hs); ms['select'].append(ss); ms['merge'].append(m); ms['correct'].append(x)
    leg = {'partitions': P, 'slots': qslots, 'table_bytes': int(lib.kbbq_kmer_table_bytes(qslots)), 'kept_pairs': npairs,
           'solid_slots': solid_slots, 'solid_bytes': int(lib.kbbq_kmer_table_bytes(solid_slots)), 'peak_bytes': peak, 'peak_bytes_merge': peak_solid, 'min_count': t,
           'ms_count_rounds': [round(float(np.median(v)), 3) for v in ms['count_rounds']]}
    leg['ms_count'] = round(sum(leg['ms_count_rounds']), 3)
    leg.update({'ms_' + key: round(float(np.median(ms[key])), 3) for key in ('histogram', 'select', 'merge', 'correct')})
    leg['ms_correct_all'] = [round(v, 3) for v in ms['correct']]
    assert t == plain_t and np.array_equal(hsum, plain_hist), 'the partitioned leg found another histogram'
    assert torch.equal(out, plain_out), 'the partitioned leg corrected differently'
    res['partitions'] = leg
print(json.dumps(res))
