#!/usr/bin/env python3
"""
kbbq command line -- the `recalibrate` sub-command of the reference CLI
and the `benchmark` sub-command (reference kbbq/main.py:26-89).  `plot` is out of scope here.
`bqsr` (alignments -> GATK report) and `applybqsr` (report -> recalibrated SAM) are this build's own: the reference has the
functions (kbbq/gatk/bqsr.py, applybqsr.py) but no command for them.  So is `correct` (k-mer error correction, kbbq/kmer.py):
the reference's tutorial leaves that step to an external corrector; `recalibrate -c FASTQ` is `correct` and `recalibrate -f` in
one run over one file (kbbq/recalibrate.py recalibrate_corrected), and `recalibrate -b ALN --kmers` is `bqsr --kmers` and `applybqsr`
in one run over one parse and one upload of the alignments (recalibrate_bam).
"""
import argparse

from . import __version__
from . import recalibrate as _recal


def _passes(text):
    """--passes P: an integer in 1..8 (the range of the kbbq_kmer_*_passes* calls)."""
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('%r is not an integer' % text) from None
    if not 1 <= value <= 8:
        raise argparse.ArgumentTypeError('must be in 1..8, got %d' % value)
    return value


def _partitions(text):
    """--partitions P|auto: an integer in 1..64, or the word auto (kmer.check_partitions)."""
    if text == 'auto':
        return text
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is neither an integer nor 'auto'" % text) from None
    if not 1 <= value <= 64:
        raise argparse.ArgumentTypeError('must be in 1..64, got %d' % value)
    return value


def _min_qual(text):
    """--kmer-min-qual Q: an integer in 1..93 (kmer.check_kmer_min_qual)."""
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('%r is not an integer' % text) from None
    if not 1 <= value <= 93:
        raise argparse.ArgumentTypeError('must be in 1..93, got %d' % value)
    return value


def _exclude_flags(text):
    """-F / --exclude-flags INT: SAM FLAG bits, decimal or 0x.., in 0..0xFFFF."""
    try:
        value = int(text, 16) if text.lower().startswith('0x') else int(text, 10)
    except ValueError:
        raise argparse.ArgumentTypeError('%r is not an integer (decimal or 0x..)' % text) from None
    if not 0 <= value <= 0xFFFF:
        raise argparse.ArgumentTypeError('must be in 0..0xFFFF, got %s' % text)
    return value


_EXCLUDE_HELP = ('%s: leave records with any of these FLAG bits (decimal or 0x..; default 0) out of the k-mer count and the tally '
                 '-- they teach the model nothing%s.  -F 0xF00 is the set GATK\'s BaseRecalibrator leaves out as far as SAM '
                 'flags express it: secondary, QC-fail, duplicate and supplementary records')
_MIXED_HELP = ('%s: take records of several query lengths (trimmed reads, hard-clipped supplementary records): the cycle axis is '
               'twice the longest record, the rows have its pitch')


def _quant_levels(text):
    """--static-quantized-quals Q[,Q...]: integers in 6..93 (the minscore of every apply up to the top of the FASTQ scale)."""
    levels = []
    for item in text.split(','):
        try:
            value = int(item.strip())
        except ValueError:
            raise argparse.ArgumentTypeError('%r is not an integer (Q[,Q...])' % item) from None
        if not 6 <= value <= 93:
            raise argparse.ArgumentTypeError('levels must be in 6..93, got %d' % value)
        levels.append(value)
    return levels


def _quantize(parser, args):
    """The 256-byte map of --static-quantized-quals / --round-down-quantized (gatk.applybqsr.quantize_map) as the `quantize`
    keyword of the calls below, or nothing -- then every call is the one it was.  An error of the two options is the parser's."""
    if args.static_quantized_quals is None:
        if args.round_down_quantized:
            parser.error('--round-down-quantized: only with --static-quantized-quals')
        return {}
    from .gatk.applybqsr import quantize_map
    levels = sorted({q for given in args.static_quantized_quals for q in given})
    return dict(quantize=quantize_map(levels, round_down=args.round_down_quantized))


_QUANT_HELP = ('round every quality that is written to the nearest of these levels and of 6, the quality below which bases keep '
               'theirs (ties go down): the output compresses as binned input does.  Comma-separated, 6..93; may be given more '
               'than once.  Qualities below 6, the model, a report (-g) and an OQ tag (-s) are not touched')
_ROUND_DOWN_HELP = 'with --static-quantized-quals: round down to the level below instead of to the nearest'


_PARTITIONS_HELP = ('%s: count the k-mers in this many rounds, 1..64 (default 1), each over all reads and for one hash partition of '
                    'the k-mers, through a table 1/P the size (--slots, where given, is that table); the k-mers that can be '
                    'solid are kept after each round and the reads are corrected against them: the same output, every round '
                    'hashes every k-mer.  auto: the fewest rounds whose table fits half the device budget (KBBQ_DEVICE_BUDGET).  One GPU '
                    'only: a process group splits the k-mers over its ranks already (correct --local-slots)')


_MIN_QUAL_HELP = ('%s: count only the k-mers whose bases all have quality >= Q, 1..93 (default: every k-mer): the errors sit at the '
                  'low-quality bases, so the table, sized from the counted k-mers, is several times smaller and the histogram\'s '
                  'valley is cleaner.  The reads are corrected as read: a low-quality base is trusted through the k-mers other '
                  'reads contributed.  The qualities are the ones the command reads%s')


_PASSES_HELP = ('%s: apply the k-mer rule to its own output this many times, 1..8 (default 1), read by read against the one table '
                'counted from the reads as read: an error next to a read end or to another error is corrected once its '
                'neighbour is')


_KMERS_FROM_HELP = ('%s: take the k-mers from this k-mer set (`kbbq count -o SET`) instead of counting the input\'s: k is the set\'s, '
                    '--min-count (not below the set\'s --keep) or the first valley of the set\'s histogram is the threshold, --slots '
                    'the table the set is loaded into; the same output as with the same k-mers counted here.  Not with the counting '
                    'options --prefilter, --filter-bits, --partitions, --kmer-min-qual and --local-slots%s')


def _kmers_from(parser, args, needs=None):
    """--kmers-from SET: its argparse errors, before the device or a process group is touched."""
    if args.kmers_from is None:
        return
    if needs is not None and not needs[0]:
        parser.error('--kmers-from: only with %s' % needs[1])
    given = [flag for flag, v in (('--prefilter', args.prefilter or None), ('--filter-bits', args.filter_bits),
                                  ('--partitions', args.partitions), ('--kmer-min-qual', args.kmer_min_qual),
                                  ('--local-slots', getattr(args, 'local_slots', None))) if v is not None]
    if given:
        parser.error('%s: not with --kmers-from (counting options: the k-mers come counted)' % ', '.join(given))


_ENDS_WITH_THE_COMMAND = False               # set by `python -m kbbq.main`: the process ends (main._leave) when the command has run


_BGZF_HELP = ('Write the output (-o, or stdout) as a BGZF file: gzip made of independent 64 KiB blocks, deflated on the GPU. '
              'Under a launcher every FILE.rankNNNN is a complete BGZF file and the files joined in rank order inflate to the '
              'one-process bytes.  Without the option the output is plain text whatever its name.')


def _bgzf_kw(args):
    """{'bgzf': True} with --bgzf, else {}: without the option every call is the one it was."""
    return {'bgzf': True} if getattr(args, 'bgzf', False) else {}


_BAM_OUT_HELP = ('Write the output (-o, or stdout) as a BAM file, whatever its name: the records are assembled and deflated on the '
                 'GPU, and the uncompressed stream is the one the SAM text without the option defines.  One GPU; not with --bgzf.  '
                 'Without the option the output is SAM text and a .bam name is refused.')


def _bam_out_kw(args):
    """{'bam_out': True} with --bam-out, else {}: without the option every call is the one it was."""
    return {'bam_out': True} if getattr(args, 'bam_out', False) else {}


def _refuse_bam_out_ranks(args):
    """--bam-out under a launcher: refused before the process group is joined."""
    from . import parallel
    if getattr(args, 'bam_out', False) and parallel.launched_from_env():
        from .gatk.applybqsr import BAM_OUT_RANKS
        raise ValueError(BAM_OUT_RANKS)


def _recalibrate_bam_kmers(args):
    """`recalibrate -b ALN --kmers`: `bqsr --kmers` and `applybqsr` in one run (kbbq/recalibrate.py recalibrate_bam)."""
    import os
    import sys
    from . import kmer, parallel
    kmers = dict(k=31 if args.kmer is None else args.kmer, min_count=args.min_count, slots=args.slots, prefilter=args.prefilter,
                 filter_bits=4 if args.filter_bits is None else args.filter_bits)
    if args.skip_unresolved:                     # without the flag or the option the call is the one without it, as `bqsr`'s
        kmers['skip_unresolved'] = True
    if args.passes is not None:
        kmers['passes'] = args.passes
    if args.partitions is not None:
        kmers['partitions'] = args.partitions
    if args.mixed_lengths:
        kmers['mixed_lengths'] = True
    if args.exclude_flags:
        kmers['exclude_flags'] = args.exclude_flags
    if args.kmer_min_qual is not None:
        kmers['kmer_min_qual'] = args.kmer_min_qual
    if args.kmers_from is not None:
        kmers.update(kmers_from=args.kmers_from, k=args.kmer)                # k: the set's, unless -k names it
    records = {key: kmers[key] for key in ('mixed_lengths', 'exclude_flags') if key in kmers}
    # every rank of a launcher refuses here, before it joins the process group
    _refuse_bam_out_ranks(args)
    _recal.check_bam_kmers(args.bam, args.gatkreport, args.output, kmers['k'], kmers['min_count'], kmers['prefilter'],
                           kmers['filter_bits'], **{key: kmers[key] for key in ('partitions', 'passes', 'exclude_flags', 'kmers_from')
                                                    if key in kmers}, **_bam_out_kw(args))
    parallel.init_from_env()
    from . import aln
    from ._trace import stage
    with stage('[recalibrate_bam, wall]'):
        with stage('parse'):
            bam = aln.AlignmentFile(args.bam)    # the one parse; what the records are refused for, before the device is touched
        _recal.check_bam_records(bam, args.use_oq, 31 if kmers['k'] is None else kmers['k'], kmers['min_count'], kmers['prefilter'],
                                 kmers['filter_bits'], **records)
        if kmer._ranks() is None and 'torch' not in sys.modules and not os.environ.get('KBBQ_USE_TORCH'):
            from . import _device
            _device.use_native_memory()          # as `bqsr --kmers` on one GPU: no torch import
        info = _recal.recalibrate_bam(bam, use_oq=args.use_oq, set_oq=args.set_oq, kmers=kmers, gatkreport=args.gatkreport,
                                      output=args.output, **args.quantize, **_bgzf_kw(args), **_bam_out_kw(args))
    sys.stderr.write('kbbq recalibrate: k=%d min_count=%d reads=%d%s flagged_bases=%d%s%s%s%s%s%s\n'
                     % (info['k'], info['min_count'], info['reads'],
                        ' excluded_reads=%d' % info['excluded_reads'] if args.exclude_flags else '', info['flagged_bases'],
                        ' skipped_bases=%d' % info['skipped_bases'] if args.skip_unresolved else '',
                        ' passes=%d' % args.passes if (args.passes or 1) > 1 else '', kmer.partitions_field(info),
                        kmer.min_qual_field(info),
                        ' prefilter=1 admitted=%d slots=%d' % (info['admitted'], info['slots']) if args.prefilter else '',
                        kmer.kmers_from_field(info)))


def recalibrate(args):
    import os
    from . import parallel
    if args.kmers:
        return _recalibrate_bam_kmers(args)
    kopts = None
    if args.correct is not None:
        kopts = dict(k=31 if args.kmer is None else args.kmer, min_count=args.min_count, slots=args.slots, prefilter=args.prefilter,
                     filter_bits=4 if args.filter_bits is None else args.filter_bits)
        if args.fix_n:                           # without the flag the call is the one it was
            kopts['fix_n'] = True
        if args.passes is not None:
            kopts['passes'] = args.passes
        if args.skip_unresolved:
            kopts['skip_unresolved'] = True
        if args.kmer_min_qual is not None:
            kopts['kmer_min_qual'] = args.kmer_min_qual
        if args.kmers_from is not None:
            kopts.update(kmers_from=args.kmers_from, k=args.kmer)            # k: the set's, unless -k names it
        more = {}
        if args.partitions is not None:
            kopts['partitions'] = args.partitions
            more = dict(partitions=args.partitions)
        # every rank of a launcher refuses here, before it joins the process group
        _recal.check_corrected(args.correct, args.gatkreport, 31 if kopts['k'] is None else kopts['k'], kopts['min_count'],
                               kopts['prefilter'], kopts['filter_bits'], **more)
    world, _ = parallel.init_from_env()          # one process per GPU under torch.distributed.run; no-op otherwise
    if world == 1 and 'torch' not in __import__('sys').modules and not os.environ.get('KBBQ_USE_TORCH'):
        # one GPU: nothing of PyTorch is needed -- device memory, page-locked slabs, copies and events come from the library's
        # own C ABI (kbbq/_hipmem.py) and `import torch` (~1 s with its HIP context) never happens
        from . import _device, _hipmem, fastx
        _device.use_native_memory()
        if _ENDS_WITH_THE_COMMAND and not os.environ.get('KBBQ_SLOW_EXIT'):
            # this process ends right after its last byte (_leave): what it holds goes with it instead of being returned piece by piece
            _hipmem.cuda.keep_released_memory(True)
            fastx.LEAVE_OPEN = True
    if kopts is not None:
        import sys
        from ._trace import stage
        with stage('[recalibrate_corrected, wall]'):
            info = _recal.recalibrate_corrected(args.correct, infer_rg=args.infer_rg, gatkreport=args.gatkreport, output=args.output,
                                                **kopts, **args.quantize, **_bgzf_kw(args))
        from .kmer import kmers_from_field, min_qual_field, partitions_field
        sys.stderr.write('kbbq recalibrate: k=%d min_count=%d reads=%d changed_bases=%d%s%s%s%s%s%s%s\n'
                         % (info['k'], info['min_count'], info['reads'], info['changed_bases'],
                            ' skipped_bases=%d' % info['skipped_bases'] if kopts.get('skip_unresolved') else '',
                            ' fix_n=1' if kopts.get('fix_n') else '',
                            ' passes=%d' % kopts['passes'] if kopts.get('passes', 1) > 1 else '', partitions_field(info),
                            min_qual_field(info),
                            ' prefilter=1 admitted=%d slots=%d' % (info['admitted'], info['slots']) if kopts['prefilter'] else '',
                            kmers_from_field(info)))
        return
    _recal.recalibrate(bam=args.bam, fastq=args.fastq, infer_rg=args.infer_rg,
                       use_oq=args.use_oq, set_oq=args.set_oq, gatkreport=args.gatkreport, output=args.output, **args.quantize,
                       **_bgzf_kw(args))


def benchmark(args):
    from . import benchmark as _bm
    from . import parallel
    parallel.init_from_env()          # one process per GPU under torch.distributed.run; no-op otherwise
    kmers = {}
    if args.kmers:                                                             # without the flag the call is what it was
        kmers = dict(kmers=dict(k=31 if args.kmer is None else args.kmer, min_count=args.min_count, slots=args.slots,
                                prefilter=args.prefilter, filter_bits=4 if args.filter_bits is None else args.filter_bits))
        if args.passes is not None:
            kmers['kmers']['passes'] = args.passes
        if args.partitions is not None:
            kmers['kmers']['partitions'] = args.partitions
        if args.kmer_min_qual is not None:
            kmers['kmers']['kmer_min_qual'] = args.kmer_min_qual
        if args.kmers_from is not None:
            kmers['kmers'].update(kmers_from=args.kmers_from, k=args.kmer)   # k: the set's, unless -k names it
    _bm.benchmark(bamfile=args.bam, fafile=args.reference, vcffile=args.vcf, fastqfile=args.fastq,
                  label=args.label, use_oq=args.use_oq, bedfh=args.bedfile, **kmers)


def applybqsr(args):
    from . import parallel
    from .gatk import applybqsr as _apply
    _refuse_bam_out_ranks(args)
    parallel.init_from_env()          # one process per GPU under torch.distributed.run; no-op otherwise
    _apply.apply_report(args.bam, args.gatkreport, use_oq=args.use_oq, set_oq=args.set_oq, output=args.output, **args.quantize,
                        **_bgzf_kw(args), **_bam_out_kw(args))


def bqsr(args):
    from . import aln
    from .gatk import bqsr as _bqsr
    if args.kmers:
        import os
        import sys
        from . import kmer, parallel
        parallel.init_from_env()             # under a launcher every rank joins its group, and bam_to_kmer_covariates refuses on each
        if kmer._ranks() is None and 'torch' not in sys.modules and not os.environ.get('KBBQ_USE_TORCH'):
            from . import _device
            _device.use_native_memory()      # as `correct` on one GPU: no torch import
        info = {}
        skip = dict(skip_unresolved=True) if args.skip_unresolved else {}      # without the flag the call is what it was
        more = dict(passes=args.passes) if args.passes is not None else {}     # ... and without this option
        if args.partitions is not None:
            more['partitions'] = args.partitions
        if args.mixed_lengths:
            more['mixed_lengths'] = True
        if args.exclude_flags:
            more['exclude_flags'] = args.exclude_flags
        if args.kmer_min_qual is not None:
            more['kmer_min_qual'] = args.kmer_min_qual
        if args.kmers_from is not None:
            more['kmers_from'] = args.kmers_from
        _bqsr.bam_to_report_kmers(aln.AlignmentFile(args.bam),
                                  k=args.kmer if args.kmers_from is not None or args.kmer is not None else 31, min_count=args.min_count,
                                  slots=args.slots, prefilter=args.prefilter,
                                  filter_bits=4 if args.filter_bits is None else args.filter_bits, use_oq=args.use_oq,
                                  info=info, **skip, **more).write(args.gatkreport)
        sys.stderr.write('kbbq bqsr: k=%d min_count=%d reads=%d%s flagged_bases=%d%s%s%s%s%s%s\n'
                         % (info['k'], info['min_count'], info['reads'],
                            ' excluded_reads=%d' % info['excluded_reads'] if args.exclude_flags else '', info['flagged_bases'],
                            ' skipped_bases=%d' % info['skipped_bases'] if skip else '',
                            ' passes=%d' % args.passes if (args.passes or 1) > 1 else '', kmer.partitions_field(info),
                            kmer.min_qual_field(info),
                            ' prefilter=1 admitted=%d slots=%d' % (info['admitted'], info['slots']) if args.prefilter else '',
                            kmer.kmers_from_field(info)))
        return
    from . import benchmark as _bm
    _bqsr.bam_to_report(aln.AlignmentFile(args.bam), args.reference, _bm.get_var_sites(args.vcf)).write(args.gatkreport)


def correct(args):
    import os
    import sys
    if 'RANK' in os.environ:
        from . import parallel
        parallel.init_from_env()             # one process per GPU under torch.distributed.run; no-op for a single rank
    elif int(os.environ.get('WORLD_SIZE', '1')) > 1:
        sys.exit('kbbq correct: WORLD_SIZE > 1 but no RANK: start one process per GPU with torch.distributed.run, or run '
                 'it on one GPU without WORLD_SIZE')
    from . import kmer
    if 'torch' not in sys.modules and not os.environ.get('KBBQ_USE_TORCH'):
        from . import _device
        _device.use_native_memory()          # as `recalibrate` on one GPU: no torch import
    more = dict(passes=args.passes) if args.passes is not None else {}         # without the option the call is what it was
    if args.partitions is not None:
        more['partitions'] = args.partitions
    if args.kmer_min_qual is not None:
        more['kmer_min_qual'] = args.kmer_min_qual
    if args.kmers_from is not None:
        more['kmers_from'] = args.kmers_from
    kmer.main_correct(args.fastq, output=args.output, k=args.kmer if args.kmers_from is not None or args.kmer is not None else 31,
                      min_count=args.min_count, slots=args.slots, local_slots=args.local_slots, prefilter=args.prefilter,
                      filter_bits=4 if args.filter_bits is None else args.filter_bits, fix_n=args.fix_n, **more, **_bgzf_kw(args))


def count(args):
    import os
    import sys
    from . import kmerset
    opts = dict(k=args.kmer, keep=args.keep, slots=args.slots, prefilter=args.prefilter,
                filter_bits=4 if args.filter_bits is None else args.filter_bits, partitions=1 if args.partitions is None else args.partitions,
                kmer_min_qual=args.kmer_min_qual, use_oq=args.use_oq, exclude_flags=args.exclude_flags or 0, histo=args.histo)
    # every rank of a launcher refuses here, before it joins a process group, and everything else count refuses on its arguments
    kmerset.check_count(args.fastq, args.bam, args.output, opts['k'], opts['keep'], opts['prefilter'], opts['filter_bits'],
                        opts['partitions'], opts['kmer_min_qual'], opts['use_oq'], opts['exclude_flags'])
    if 'torch' not in sys.modules and not os.environ.get('KBBQ_USE_TORCH'):
        from . import _device
        _device.use_native_memory()          # as `correct` on one GPU: no torch import
    kmerset.main_count(args.fastq, args.bam, args.output, **opts)


def main(argv=None):
    parser = argparse.ArgumentParser(description='K-mer Based Base Quality score recalibration (MI355X build)')
    parser.add_argument('-v', '--version', action='version', version=__version__)
    sub = parser.add_subparsers(title='command', description='valid commands')
    parser.set_defaults(command=lambda a: parser.print_help)
    sub.add_parser('help', description='Print help information').set_defaults(
        command=lambda a: parser.print_help)

    rp = sub.add_parser('recalibrate', description='Recalibrate a BAM or FASTQ file')
    src = rp.add_mutually_exclusive_group(required=True)
    src.add_argument('-b', '--bam', help='BAM to recalibrate')
    src.add_argument('-f', '--fastq', nargs=2,
                     help='FASTQ file to recalibrate and an error-corrected version of it.')
    src.add_argument('-c', '--correct', metavar='FASTQ',
                     help='FASTQ file to recalibrate against its own k-mer correction, made on the GPU in the same run (not in '
                          'the reference): `kbbq correct` and `recalibrate -f` in one command, the same output, one GPU.')
    rp.add_argument('--kmers', action='store_true',
                    help='with -b: recalibrate the alignments from their own k-mers (not in the reference): `kbbq bqsr -b ALN --kmers '
                         '-g R` and `kbbq applybqsr -b ALN -g R` in one run over one parse and one upload of the file, the same SAM '
                         'text; takes the k-mer options below except --fix-n, and -u, -s, -g (the report is written there) and -o; '
                         'all records of one query length (unless --mixed-lengths), one GPU')
    rp.add_argument('--mixed-lengths', action='store_true', help=_MIXED_HELP % 'with -b --kmers')
    rp.add_argument('-F', '--exclude-flags', type=_exclude_flags, default=None, metavar='INT',
                    help=_EXCLUDE_HELP % ('with -b --kmers', '; they are still recalibrated and written like any other'))
    rp.add_argument('-k', '--kmer', type=int, default=None, help='with -c: k-mer length, 8..32 (default 31)')
    rp.add_argument('--min-count', type=int, default=None,
                    help='with -c: k-mers seen at least this often are solid (default: the first valley of the count histogram)')
    rp.add_argument('--slots', type=int, default=None,
                    help='with -c: hash table slots, a power of two (default: every k-mer of the input at a load factor of 0.5, '
                         'capped by what the device budget leaves beside the resident reads)')
    rp.add_argument('--prefilter', action='store_true',
                    help='with -c: keep most k-mers seen once out of the table (as `kbbq correct --prefilter`); needs '
                         '--min-count >= 2 where given')
    rp.add_argument('--filter-bits', type=int, default=None,
                    help='with -c --prefilter: bits per k-mer of the input in each of the filter\'s two arrays, 1..64 (default 4)')
    rp.add_argument('--fix-n', action='store_true',
                    help='with -c: give every N the letter that makes the most of the k-mers it alone breaks solid (as `kbbq '
                         'correct --fix-n`)')
    rp.add_argument('--passes', type=_passes, default=None, metavar='P', help=_PASSES_HELP % 'with -c')
    rp.add_argument('--partitions', type=_partitions, default=None, metavar='P|auto', help=_PARTITIONS_HELP % 'with -c')
    rp.add_argument('--kmer-min-qual', type=_min_qual, default=None, metavar='Q',
                    help=_MIN_QUAL_HELP % ('with -c, or with -b --kmers', ': the FASTQ quality lines, QUAL, or the OQ tag with -u'))
    rp.add_argument('--kmers-from', default=None, metavar='SET', help=_KMERS_FROM_HELP % ('with -c, or with -b --kmers', ''))
    rp.add_argument('--skip-unresolved', action='store_true',
                    help='with -c: leave a base out of the tally (neither error nor observation) when the k-mers contradict it but '
                         'name no replacement -- two errors within k bases, thin coverage, contamination -- instead of counting '
                         'it as correct (as `kbbq bqsr --kmers --skip-unresolved`)')
    rp.add_argument('-u', '--use-oq', action='store_true',
                    help='Use the OQ tag for quality scores (BAM input only).')
    rp.add_argument('-s', '--set-oq', action='store_true',
                    help="with -b --kmers: keep the qualities as read in an 'OQ' tag where there is none (SAM and BAM output).")
    rp.add_argument('-g', '--gatkreport', help='Load the model from / save it to a GATK report.')
    rp.add_argument('-o', '--output', default=None,
                    help='Write the recalibrated FASTQ to this file instead of stdout (not in the reference); under '
                         'torch.distributed.run every rank writes FILE.rankNNNN, to be concatenated in rank order.')
    rp.add_argument('--bgzf', action='store_true', help=_BGZF_HELP)
    rp.add_argument('--bam-out', action='store_true', help='with -b --kmers: ' + _BAM_OUT_HELP)
    rp.add_argument('--infer-rg', action='store_true',
                    help='Infer the read group from the FASTQ read name (name_RG:Z:id).')
    rp.add_argument('--static-quantized-quals', type=_quant_levels, action='append', default=None, metavar='Q[,Q...]',
                    help='(not in the reference) ' + _QUANT_HELP)
    rp.add_argument('--round-down-quantized', action='store_true', help=_ROUND_DOWN_HELP)
    rp.set_defaults(command=recalibrate)

    bp = sub.add_parser('benchmark', description='Benchmark a SAM or FASTQ file using a truth set')
    req = bp.add_argument_group(title='required arguments')
    req.add_argument('-b', '--bam', required=True,
                     help='Truth set alignments (SAM text). Differences from the reference at nonvariable sites are errors.')
    req.add_argument('-r', '--reference', required=True, help='FASTA file containing the reference genome')
    req.add_argument('-v', '--vcf', required=True, help='VCF file containing variable sites')
    bp.add_argument('-f', '--fastq', default=None, help='fastq file to benchmark')
    bp.add_argument('-l', '--label', default=None, help='label to use for label column')
    bp.add_argument('-u', '--use-oq', action='store_true', help='Use the OQ tag for quality scores')
    bp.add_argument('-d', '--bedfile', type=argparse.FileType('r'),
                    help='BED file of confident regions. Sites outside the given regions will be skipped.')
    bp.add_argument('--kmers', action='store_true',
                    help='score the k-mer rule of `kbbq correct` / `bqsr --kmers` against the truth set: per reported quality, '
                         'the bases the alignments\' own k-mers flag as errors or leave unresolved beside the true errors, and '
                         'the quality each reading of the flags implies; a summary with precision and recall on stderr; one '
                         'GPU, not with -f')
    bp.add_argument('-k', '--kmer', type=int, default=None, help='with --kmers: k-mer length, 8..32 (default 31)')
    bp.add_argument('--min-count', type=int, default=None,
                    help='with --kmers: k-mers seen at least this often are solid (default: the first valley of the count histogram)')
    bp.add_argument('--slots', type=int, default=None,
                    help='with --kmers: hash table slots, a power of two (default: every k-mer of the input at a load factor of '
                         '0.5, capped by what the device budget leaves beside the resident alignments)')
    bp.add_argument('--prefilter', action='store_true',
                    help='with --kmers: keep most k-mers seen once out of the table (as `kbbq correct --prefilter`); needs '
                         '--min-count >= 2 where given')
    bp.add_argument('--filter-bits', type=int, default=None,
                    help='with --kmers --prefilter: bits per k-mer of the input in each of the filter\'s two arrays, 1..64 (default 4)')
    bp.add_argument('--passes', type=_passes, default=None, metavar='P', help=_PASSES_HELP % 'with --kmers')
    bp.add_argument('--partitions', type=_partitions, default=None, metavar='P|auto', help=_PARTITIONS_HELP % 'with --kmers')
    bp.add_argument('--kmer-min-qual', type=_min_qual, default=None, metavar='Q',
                    help=_MIN_QUAL_HELP % ('with --kmers', ': QUAL, or the OQ tag with -u; a record without qualities is refused'))
    bp.add_argument('--kmers-from', default=None, metavar='SET',
                    help=_KMERS_FROM_HELP % ('with --kmers', ': the set `bqsr --kmers --kmers-from` used can be scored here'))
    bp.set_defaults(command=benchmark)

    ap = sub.add_parser('applybqsr', description='Recalibrate alignments with a GATK recalibration report (SAM output, or BAM '
                        'with --bam-out)')
    ap.add_argument('-b', '--bam', required=True, help='SAM or BAM file to recalibrate')
    ap.add_argument('-g', '--gatkreport', required=True, help='GATK recalibration report (kbbq bqsr, GATK BaseRecalibrator)')
    ap.add_argument('-o', '--output', default=None,
                    help='Write the recalibrated SAM to this file instead of stdout (SAM text; a .bam name is refused without --bam-out); '
                         'under torch.distributed.run every rank writes FILE.rankNNNN, to be concatenated in rank order.')
    ap.add_argument('--bgzf', action='store_true', help=_BGZF_HELP)
    ap.add_argument('--bam-out', action='store_true', help=_BAM_OUT_HELP)
    ap.add_argument('-u', '--use-oq', action='store_true', help='Recalibrate the OQ tag\'s qualities instead of QUAL.')
    ap.add_argument('-s', '--set-oq', action='store_true', help="Keep the qualities as read in an 'OQ' tag where there is none.")
    ap.add_argument('--static-quantized-quals', type=_quant_levels, action='append', default=None, metavar='Q[,Q...]',
                    help=_QUANT_HELP)
    ap.add_argument('--round-down-quantized', action='store_true', help=_ROUND_DOWN_HELP)
    ap.set_defaults(command=applybqsr)

    qp = sub.add_parser('bqsr', description='Build a GATK recalibration report from alignments (BaseRecalibrator): errors are '
                        'differences from a reference outside known sites (-r -v), or what the k-mers of the alignments\' own '
                        'sequences contradict (--kmers: no reference, no known sites)')
    qp.add_argument('-b', '--bam', required=True, help='SAM or BAM file (qualities from the OQ tag; with --kmers from QUAL unless -u)')
    qp.add_argument('-r', '--reference', default=None, help='FASTA file containing the reference genome (needed without --kmers)')
    qp.add_argument('-v', '--vcf', default=None, help='VCF file of known variable sites (skipped; needed without --kmers)')
    qp.add_argument('-g', '--gatkreport', required=True, help='Write the report to this file')
    qp.add_argument('--kmers', action='store_true',
                    help='take the errors from the k-mer correction of the alignments\' own sequences (as `kbbq correct` decides '
                         'them) instead of a reference and known sites; all records of one query length (unless --mixed-lengths), '
                         'one GPU')
    qp.add_argument('--mixed-lengths', action='store_true', help=_MIXED_HELP % 'with --kmers')
    qp.add_argument('-F', '--exclude-flags', type=_exclude_flags, default=None, metavar='INT', help=_EXCLUDE_HELP % ('with --kmers', ''))
    qp.add_argument('-k', '--kmer', type=int, default=None, help='with --kmers: k-mer length, 8..32 (default 31)')
    qp.add_argument('--min-count', type=int, default=None,
                    help='with --kmers: k-mers seen at least this often are solid (default: the first valley of the count histogram)')
    qp.add_argument('--slots', type=int, default=None,
                    help='with --kmers: hash table slots, a power of two (default: every k-mer of the input at a load factor of '
                         '0.5, capped by what the device budget leaves beside the resident alignments)')
    qp.add_argument('--prefilter', action='store_true',
                    help='with --kmers: keep most k-mers seen once out of the table (as `kbbq correct --prefilter`); needs '
                         '--min-count >= 2 where given')
    qp.add_argument('--filter-bits', type=int, default=None,
                    help='with --kmers --prefilter: bits per k-mer of the input in each of the filter\'s two arrays, 1..64 (default 4)')
    qp.add_argument('-u', '--use-oq', action='store_true', help='with --kmers: qualities from the OQ tag instead of QUAL')
    qp.add_argument('--skip-unresolved', action='store_true',
                    help='with --kmers: leave a base out of the tally (neither error nor observation) when the k-mers contradict '
                         'it but name no replacement -- two errors within k bases, thin coverage, contamination -- instead of '
                         'counting it as correct')
    qp.add_argument('--passes', type=_passes, default=None, metavar='P', help=_PASSES_HELP % 'with --kmers')
    qp.add_argument('--partitions', type=_partitions, default=None, metavar='P|auto', help=_PARTITIONS_HELP % 'with --kmers')
    qp.add_argument('--kmer-min-qual', type=_min_qual, default=None, metavar='Q',
                    help=_MIN_QUAL_HELP % ('with --kmers', ': QUAL, or the OQ tag with -u'))
    qp.add_argument('--kmers-from', default=None, metavar='SET',
                    help=_KMERS_FROM_HELP % ('with --kmers', ': a set counted from the raw FASTQ decides the errors of its alignments'))
    qp.set_defaults(command=bqsr)

    cp = sub.add_parser('correct', description='Correct substitution errors of a FASTQ file with k-mer counts (GPU); the output '
                        'is the error-corrected file `recalibrate -f` takes')
    cp.add_argument('-f', '--fastq', required=True, help='FASTQ file to correct (plain or .gz)')
    cp.add_argument('-k', '--kmer', type=int, default=None, help='k-mer length, 8..32 (default 31)')
    cp.add_argument('--min-count', type=int, default=None,
                    help='k-mers seen at least this often are solid (default: the first valley of the count histogram)')
    cp.add_argument('--slots', type=int, default=None,
                    help='hash table slots, a power of two (default: every k-mer of the input at a load factor of 0.5, '
                         'capped by the device budget); under torch.distributed.run: the slots of every rank\'s share of the '
                         'k-mers (default: the input\'s k-mers / ranks * 9/8 at a load factor of 0.5)')
    cp.add_argument('--local-slots', type=int, default=None,
                    help='under torch.distributed.run: slots of the table every rank counts its own reads into before they go '
                         'to the ranks that own them, a power of two (default: the rank\'s k-mers at a load factor of 0.5, '
                         'capped by half the device budget); a smaller table counts the reads in several rounds')
    cp.add_argument('--prefilter', action='store_true',
                    help='keep most k-mers seen once out of the table with a bit filter passed over the reads first: the same '
                         'output from a table several times smaller, sized from the filter unless --slots is given; needs '
                         '--min-count >= 2 where given; one GPU only (not under torch.distributed.run)')
    cp.add_argument('--filter-bits', type=int, default=None,
                    help='with --prefilter: bits per k-mer of the input in each of the filter\'s two arrays, 1..64 (default 4)')
    cp.add_argument('--fix-n', action='store_true',
                    help='give every N the letter (A, C, G or T) that makes the most of the k-mers it alone breaks solid; an N '
                         'stays N on a tie or when no letter makes a solid k-mer; a fixed N counts as a changed base')
    cp.add_argument('--passes', type=_passes, default=None, metavar='P', help=_PASSES_HELP % 'the whole rule (with --fix-n the N rule too)')
    cp.add_argument('--partitions', type=_partitions, default=None, metavar='P|auto', help=_PARTITIONS_HELP % 'one GPU')
    cp.add_argument('--kmer-min-qual', type=_min_qual, default=None, metavar='Q',
                    help=_MIN_QUAL_HELP % ('one GPU or several', ': the FASTQ quality lines'))
    cp.add_argument('-o', '--output', default=None,
                    help='Write the corrected FASTQ to this file instead of stdout; under torch.distributed.run every rank '
                         'writes FILE.rankNNNN, to be concatenated in rank order.')
    cp.add_argument('--bgzf', action='store_true', help=_BGZF_HELP)
    cp.add_argument('--kmers-from', default=None, metavar='SET',
                    help=_KMERS_FROM_HELP % ('one GPU or several', '; under torch.distributed.run every rank loads the set'))
    cp.set_defaults(command=correct)

    np_ = sub.add_parser('count', description='Count the k-mers of one or several FASTQ and alignment files into one k-mer set (GPU): '
                         'the file --kmers-from of correct, recalibrate -c, bqsr --kmers, recalibrate -b --kmers and benchmark '
                         '--kmers takes in the place of their own count.  One input is resident at a time; one GPU')
    np_.add_argument('-f', '--fastq', nargs='+', default=[], metavar='FASTQ',
                     help='FASTQ files (plain or .gz), counted as `kbbq correct` counts its input')
    np_.add_argument('-b', '--bam', nargs='+', default=[], metavar='ALN',
                     help='SAM or BAM files, counted as `kbbq bqsr --kmers` counts its input: every base of SEQ, soft clips included; '
                          'records of any lengths')
    np_.add_argument('-o', '--output', default=None, metavar='SET', help='the k-mer set to write; an existing file is refused')
    np_.add_argument('-k', '--kmer', type=int, default=31, help='k-mer length, 8..32 (default 31)')
    np_.add_argument('--keep', type=int, default=2,
                     help='write the k-mers seen at least this often (default 2, the smallest threshold the histogram\'s valley can '
                          'give); a --min-count below it cannot be served from the set; >= 2 with --prefilter')
    np_.add_argument('--slots', type=int, default=None,
                     help='hash table slots, a power of two (default: every k-mer of all inputs at a load factor of 0.5, capped by '
                          'the device budget; with --partitions: the table of one round)')
    np_.add_argument('--prefilter', action='store_true',
                     help='keep most k-mers seen once out of the table (as `kbbq correct --prefilter`): the filter pass runs over all '
                          'inputs, then the count; the same set')
    np_.add_argument('--filter-bits', type=int, default=None,
                     help='with --prefilter: bits per k-mer of the inputs in each of the filter\'s two arrays, 1..64 (default 4)')
    np_.add_argument('--partitions', type=_partitions, default=None, metavar='P|auto',
                     help=_PARTITIONS_HELP % 'every round over all inputs')
    np_.add_argument('--kmer-min-qual', type=_min_qual, default=None, metavar='Q',
                     help=_MIN_QUAL_HELP % ('every input', ': the FASTQ quality lines, QUAL, or the OQ tag with -u'))
    np_.add_argument('-u', '--use-oq', action='store_true', help='with -b and --kmer-min-qual: gate by the OQ tag instead of QUAL')
    np_.add_argument('-F', '--exclude-flags', type=_exclude_flags, default=None, metavar='INT', help=_EXCLUDE_HELP % ('with -b', ''))
    np_.add_argument('--histo', default=None, metavar='FILE',
                     help='write the count histogram as `count<TAB>k-mers` lines for counts --keep..256 (the last line: 256 and more), '
                          'the shape Jellyfish prints and GenomeScope reads')
    np_.set_defaults(command=count)

    args = parser.parse_args(argv)
    if args.command is correct:
        _kmers_from(cp, args)
    elif args.command is recalibrate:
        _kmers_from(rp, args, (args.correct is not None or (args.kmers and args.bam is not None), '-c/--correct or with -b --kmers'))
    elif args.command is bqsr or args.command is benchmark:
        _kmers_from(qp if args.command is bqsr else bp, args, (args.kmers, '--kmers'))
    elif args.command is count:
        # decided here: before the device is touched and, under a launcher, before a process group could exist
        if not args.fastq and not args.bam:
            np_.error('at least one input is required: -f FASTQ [FASTQ ...] and / or -b ALN [ALN ...]')
        if args.output is None:
            np_.error('the following arguments are required: -o/--output')
        given = [flag for flag, v in (('-u/--use-oq', args.use_oq or None), ('-F/--exclude-flags', args.exclude_flags)) if v is not None]
        if given and not args.bam:
            np_.error('%s: only with -b' % ', '.join(given))
    if args.command is recalibrate or args.command is applybqsr:
        # decided here: before the device is touched and, under a launcher, before the process group exists
        args.quantize = _quantize(rp if args.command is recalibrate else ap, args)
        if args.bam_out and args.bgzf:
            (rp if args.command is recalibrate else ap).error('--bam-out: not with --bgzf (a BAM file is a BGZF file already)')
        if args.bam_out and args.command is recalibrate and not (args.kmers and args.bam is not None):
            rp.error('--bam-out: only with -b --kmers')
    if args.command is recalibrate and not (args.kmers and args.bam is not None):
        given = [flag for flag, v in (('--mixed-lengths', args.mixed_lengths or None), ('-F/--exclude-flags', args.exclude_flags))
                 if v is not None]
        if given:
            rp.error('%s: only with -b --kmers' % ', '.join(given))
    if args.command is recalibrate and args.kmer_min_qual is not None and args.correct is None \
            and not (args.kmers and args.bam is not None):
        rp.error('--kmer-min-qual: only with -c/--correct or with -b --kmers')
    if args.command is recalibrate and args.kmers:
        if args.bam is None:
            rp.error('--kmers: only with -b/--bam (-c/--correct corrects and recalibrates a FASTQ file)')
        given = [flag for flag, v in (('--fix-n', args.fix_n), ('--infer-rg', args.infer_rg)) if v]
        if given:
            rp.error('%s: not with -b --kmers (FASTQ input only)' % ', '.join(given))
    elif args.command is recalibrate and args.correct is None:
        given = [flag for flag, v in (('-k/--kmer', args.kmer), ('--min-count', args.min_count), ('--slots', args.slots),
                                      ('--prefilter', args.prefilter or None), ('--filter-bits', args.filter_bits),
                                      ('--fix-n', args.fix_n or None), ('--passes', args.passes),
                                      ('--skip-unresolved', args.skip_unresolved or None),
                                      ('--partitions', args.partitions)) if v is not None]
        if given:
            rp.error('%s: only with -c/--correct' % ', '.join(given))
    if args.command is benchmark:
        if args.kmers:
            if args.fastq is not None:
                bp.error('-f/--fastq: not with --kmers (the k-mers are those of the alignments\' own sequences)')
        else:
            given = [flag for flag, v in (('-k/--kmer', args.kmer), ('--min-count', args.min_count), ('--slots', args.slots),
                                          ('--prefilter', args.prefilter or None), ('--filter-bits', args.filter_bits),
                                          ('--passes', args.passes), ('--partitions', args.partitions),
                                          ('--kmer-min-qual', args.kmer_min_qual)) if v is not None]
            if given:
                bp.error('%s: only with --kmers' % ', '.join(given))
    if args.command is bqsr:
        if args.kmers:
            given = [flag for flag, v in (('-r/--reference', args.reference), ('-v/--vcf', args.vcf)) if v is not None]
            if given:
                qp.error('%s: not with --kmers (its errors come from the alignments\' own k-mers)' % ', '.join(given))
        else:
            given = [flag for flag, v in (('-k/--kmer', args.kmer), ('--min-count', args.min_count), ('--slots', args.slots),
                                          ('--prefilter', args.prefilter or None), ('--filter-bits', args.filter_bits),
                                          ('-u/--use-oq', args.use_oq or None),
                                          ('--skip-unresolved', args.skip_unresolved or None), ('--passes', args.passes),
                                          ('--partitions', args.partitions), ('--mixed-lengths', args.mixed_lengths or None),
                                          ('-F/--exclude-flags', args.exclude_flags), ('--kmer-min-qual', args.kmer_min_qual))
                     if v is not None]
            if given:
                qp.error('%s: only with --kmers' % ', '.join(given))
            missing = [flag for flag, v in (('-r/--reference', args.reference), ('-v/--vcf', args.vcf)) if v is None]
            if missing:
                qp.error('the following arguments are required: %s' % ', '.join(missing))
    args.command(args)


def _leave():
    """The command's last step when it ran as a single process without torch: flush, run the exit handlers (the stage report of
    KBBQ_TIMING) and end the process without taking it apart piece by piece -- unmapping 5 GB of input, returning a gigabyte of
    page-locked buffers and shutting the HIP runtime down cost the command 0.1-0.2 s after its last byte was written; the
    kernel releases all of it faster.  Under a launcher (torch imported: process group, RCCL) the ordinary exit stays."""
    import atexit
    import os
    import sys
    if 'torch' in sys.modules or os.environ.get('KBBQ_SLOW_EXIT'):
        return
    code = 0
    try:
        sys.stdout.flush()
        sys.stderr.flush()
        atexit._run_exitfuncs()
        sys.stdout.flush()
        sys.stderr.flush()
    except BaseException:                    # noqa: BLE001 -- a flush that fails (closed pipe, full disk) must not look like success:
        code = 120                           # the status the interpreter itself leaves with when its final flush fails
    os._exit(code)


if __name__ == '__main__':
    _ENDS_WITH_THE_COMMAND = True
    main()
    _leave()
