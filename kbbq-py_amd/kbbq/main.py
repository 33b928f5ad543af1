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


# ---- the k-mer options: six commands take them (recalibrate -c, recalibrate -b --kmers, bqsr --kmers, benchmark --kmers, correct, count)
#
# dest: (flags, argparse keywords, help template).  A template takes %(scope)s -- the command's `with ...: `, or nothing --,
# %(with)s -- the same words in front of another flag -- and %(more)s, the words of one command (_COMMANDS[...]['help']).
# The order of the rows is the order of the flags in a refusal.

_KMER_OPTIONS = {
    'kmer': (('-k', '--kmer'), dict(type=int, default=None), '%(scope)sk-mer length, 8..32 (default 31)'),
    'min_count': (('--min-count',), dict(type=int, default=None),
                  '%(scope)sk-mers seen at least this often are solid (default: the first valley of the count histogram)'),
    'slots': (('--slots',), dict(type=int, default=None), '%(scope)shash table slots, a power of two (default: every k-mer of %(more)s)'),
    'prefilter': (('--prefilter',), dict(action='store_true'), '%(scope)skeep most k-mers seen once out of the table%(more)s'),
    'filter_bits': (('--filter-bits',), dict(type=int, default=None),
                    '%(with)s--prefilter: bits per k-mer of the input%(more)s in each of the filter\'s two arrays, 1..64 (default 4)'),
    'fix_n': (('--fix-n',), dict(action='store_true'), '%(scope)sgive every N the letter%(more)s'),
    'passes': (('--passes',), dict(type=_passes, default=None, metavar='P'),
               '%(scope)sapply the k-mer rule to its own output this many times, 1..8 (default 1), read by read against the one table '
               'counted from the reads as read: an error next to a read end or to another error is corrected once its '
               'neighbour is'),
    'skip_unresolved': (('--skip-unresolved',), dict(action='store_true'),
                        '%(scope)sleave a base out of the tally (neither error nor observation) when the k-mers contradict it but '
                        'name no replacement -- two errors within k bases, thin coverage, contamination -- instead of counting '
                        'it as correct%(more)s'),
    'partitions': (('--partitions',), dict(type=_partitions, default=None, metavar='P|auto'),
                   '%(scope)scount the k-mers in this many rounds, 1..64 (default 1), each over all reads and for one hash partition of '
                   'the k-mers, through a table 1/P the size (--slots, where given, is that table); the k-mers that can be '
                   'solid are kept after each round and the reads are corrected against them: the same output, every round '
                   'hashes every k-mer.  auto: the fewest rounds whose table fits half the device budget (KBBQ_DEVICE_BUDGET).  One GPU '
                   'only: a process group splits the k-mers over its ranks already (correct --local-slots)'),
    'mixed_lengths': (('--mixed-lengths',), dict(action='store_true'),
                      '%(scope)stake records of several query lengths (trimmed reads, hard-clipped supplementary records): the cycle '
                      'axis is twice the longest record, the rows have its pitch'),
    'exclude_flags': (('-F', '--exclude-flags'), dict(type=_exclude_flags, default=None, metavar='INT'),
                      '%(scope)sleave records with any of these FLAG bits (decimal or 0x..; default 0) out of the k-mer count and the '
                      'tally -- they teach the model nothing%(more)s.  -F 0xF00 is the set GATK\'s BaseRecalibrator leaves out as far '
                      'as SAM flags express it: secondary, QC-fail, duplicate and supplementary records'),
    'kmer_min_qual': (('--kmer-min-qual',), dict(type=_min_qual, default=None, metavar='Q'),
                      '%(scope)scount only the k-mers whose bases all have quality >= Q, 1..93 (default: every k-mer): the errors sit at '
                      'the low-quality bases, so the table, sized from the counted k-mers, is several times smaller and the '
                      'histogram\'s valley is cleaner.  The reads are corrected as read: a low-quality base is trusted through the '
                      'k-mers other reads contributed.  The qualities are the ones the command reads%(more)s'),
    'kmers_from': (('--kmers-from',), dict(default=None, metavar='SET'),
                   '%(scope)stake the k-mers from this k-mer set (`kbbq count -o SET`) instead of counting the input\'s: k is the set\'s, '
                   '--min-count (not below the set\'s --keep) or the first valley of the set\'s histogram is the threshold, --slots '
                   'the table the set is loaded into; the same output as with the same k-mers counted here.  Not with the counting '
                   'options --prefilter, --filter-bits, --partitions, --kmer-min-qual and --local-slots%(more)s'),
    'local_slots': (('--local-slots',), dict(type=int, default=None),
                    'under torch.distributed.run: slots of the table every rank counts its own reads into before they go '
                    'to the ranks that own them, a power of two (default: the rank\'s k-mers at a load factor of 0.5, '
                    'capped by half the device budget); a smaller table counts the reads in several rounds'),
}

_COUNTING_OPTIONS = ('prefilter', 'filter_bits', 'partitions', 'kmer_min_qual', 'local_slots')      # not with --kmers-from
_SLOTS_BESIDE = 'the input at a load factor of 0.5, capped by what the device budget leaves beside the resident %s'
_PREFILTER_AS_CORRECT = ' (as `kbbq correct --prefilter`); needs --min-count >= 2 where given'
_QUAL_OR_OQ = ': QUAL, or the OQ tag with -u'


def _with_c(a):
    return a.correct is not None


def _with_b_kmers(a):
    return bool(a.kmers and a.bam is not None)


def _with_kmers(a):
    return a.kmers


# command: options -- the k-mer options it takes, in the order of its --help; scope -- what its templates say before the colon
# (help[dest]['scope']: what one option says instead); help[dest]['more'] -- the words of this command in one template;
# default -- argparse defaults that are this command's own; always -- the optional keywords its library call gets given or not
# (_kmer_kw); only_with -- (dests, is the mode on?, the mode's words): `FLAG, FLAG: only with WORDS`, in this order (_validate).
_BOTH_MODES = 'with -c, or with -b --kmers'
_COMMANDS = {
    'recalibrate': dict(
        options=('mixed_lengths', 'exclude_flags', 'kmer', 'min_count', 'slots', 'prefilter', 'filter_bits', 'fix_n', 'passes',
                 'partitions', 'kmer_min_qual', 'kmers_from', 'skip_unresolved'),
        scope='with -c',
        help=dict(mixed_lengths=dict(scope='with -b --kmers'),
                  exclude_flags=dict(scope='with -b --kmers', more='; they are still recalibrated and written like any other'),
                  slots=dict(more=_SLOTS_BESIDE % 'reads'), prefilter=dict(more=_PREFILTER_AS_CORRECT),
                  fix_n=dict(more=' that makes the most of the k-mers it alone breaks solid (as `kbbq correct --fix-n`)'),
                  kmer_min_qual=dict(scope=_BOTH_MODES, more=': the FASTQ quality lines, QUAL, or the OQ tag with -u'),
                  kmers_from=dict(scope=_BOTH_MODES), skip_unresolved=dict(more=' (as `kbbq bqsr --kmers --skip-unresolved`)')),
        only_with=((('kmers_from',), lambda a: _with_c(a) or _with_b_kmers(a), '-c/--correct or with -b --kmers'),
                   (('bam_out', 'bam_index'), _with_b_kmers, '-b --kmers'),
                   (('mixed_lengths', 'exclude_flags'), _with_b_kmers, '-b --kmers'),
                   (('kmer_min_qual',), lambda a: _with_c(a) or _with_b_kmers(a), '-c/--correct or with -b --kmers'),
                   (('kmers',), lambda a: a.bam is not None, '-b/--bam (-c/--correct corrects and recalibrates a FASTQ file)'),
                   (('kmer', 'min_count', 'slots', 'prefilter', 'filter_bits', 'fix_n', 'passes', 'skip_unresolved', 'partitions'),
                    lambda a: _with_c(a) or a.kmers, '-c/--correct'))),
    'benchmark': dict(
        options=('kmer', 'min_count', 'slots', 'prefilter', 'filter_bits', 'passes', 'partitions', 'kmer_min_qual', 'kmers_from'),
        scope='with --kmers',
        help=dict(slots=dict(more=_SLOTS_BESIDE % 'alignments'), prefilter=dict(more=_PREFILTER_AS_CORRECT),
                  kmer_min_qual=dict(more=_QUAL_OR_OQ + '; a record without qualities is refused'),
                  kmers_from=dict(more=': the set `bqsr --kmers --kmers-from` used can be scored here')),
        only_with=((('kmers_from',), _with_kmers, '--kmers'),
                   (('kmer', 'min_count', 'slots', 'prefilter', 'filter_bits', 'passes', 'partitions', 'kmer_min_qual'),
                    _with_kmers, '--kmers'))),
    'bqsr': dict(
        options=('mixed_lengths', 'exclude_flags', 'kmer', 'min_count', 'slots', 'prefilter', 'filter_bits', 'skip_unresolved', 'passes',
                 'partitions', 'kmer_min_qual', 'kmers_from'),
        scope='with --kmers',
        help=dict(slots=dict(more=_SLOTS_BESIDE % 'alignments'), prefilter=dict(more=_PREFILTER_AS_CORRECT),
                  kmer_min_qual=dict(more=_QUAL_OR_OQ),
                  kmers_from=dict(more=': a set counted from the raw FASTQ decides the errors of its alignments')),
        only_with=((('kmers_from',), _with_kmers, '--kmers'),
                   (('kmer', 'min_count', 'slots', 'prefilter', 'filter_bits', 'use_oq', 'passes', 'skip_unresolved', 'partitions',
                     'mixed_lengths', 'exclude_flags', 'kmer_min_qual'), _with_kmers, '--kmers'))),
    'correct': dict(
        options=('kmer', 'min_count', 'slots', 'local_slots', 'prefilter', 'filter_bits', 'fix_n', 'passes', 'partitions',
                 'kmer_min_qual', 'kmers_from'),
        scope='',
        help=dict(slots=dict(more='the input at a load factor of 0.5, capped by the device budget); under torch.distributed.run: the '
                                  'slots of every rank\'s share of the k-mers (default: the input\'s k-mers / ranks * 9/8 at a load '
                                  'factor of 0.5'),
                  prefilter=dict(more=' with a bit filter passed over the reads first: the same output from a table several times '
                                      'smaller, sized from the filter unless --slots is given; needs --min-count >= 2 where given; '
                                      'one GPU only (not under torch.distributed.run)'),
                  fix_n=dict(more=' (A, C, G or T) that makes the most of the k-mers it alone breaks solid; an N stays N on a tie or '
                                  'when no letter makes a solid k-mer; a fixed N counts as a changed base'),
                  passes=dict(scope='the whole rule (with --fix-n the N rule too)'), partitions=dict(scope='one GPU'),
                  kmer_min_qual=dict(scope='one GPU or several', more=': the FASTQ quality lines'),
                  kmers_from=dict(scope='one GPU or several', more='; under torch.distributed.run every rank loads the set')),
        always=('local_slots', 'fix_n'),
        only_with=()),
    'count': dict(
        options=('kmer', 'slots', 'prefilter', 'filter_bits', 'partitions', 'kmer_min_qual', 'exclude_flags'),
        scope='',
        help=dict(slots=dict(more='all inputs at a load factor of 0.5, capped by the device budget; with --partitions: the table of '
                                  'one round'),
                  prefilter=dict(more=' (as `kbbq correct --prefilter`): the filter pass runs over all inputs, then the count; the '
                                      'same set'),
                  filter_bits=dict(more='s'), partitions=dict(scope='every round over all inputs'),
                  kmer_min_qual=dict(scope='every input', more=': the FASTQ quality lines, QUAL, or the OQ tag with -u'),
                  exclude_flags=dict(scope='with -b')),
        default=dict(kmer=31),
        only_with=((('use_oq', 'exclude_flags'), lambda a: a.bam, '-b'),)),
}


def _add_kmer_options(parser, command, first=None, last=None):
    """The k-mer options of `command` from the two tables, in the order of its row: all of them, or those from `first`
    through `last` where options of the command's own stand in between."""
    row = _COMMANDS[command]
    options = row['options']
    for dest in options[options.index(first) if first else 0:options.index(last) + 1 if last else None]:
        flags, keywords, template = _KMER_OPTIONS[dest]
        words = dict(dict(scope=row['scope'], more=''), **row['help'].get(dest, {}))
        scope = words['scope']
        text = template % {'scope': scope + ': ' if scope else '', 'with': scope + ' ' if scope else 'with ', 'more': words['more']}
        if dest in row.get('default', {}):
            keywords = dict(keywords, default=row['default'][dest])
        parser.add_argument(*flags, help=text, **keywords)


def _k(args):
    return 31 if args.kmer is None else args.kmer


def _filter_bits(args):
    return 4 if args.filter_bits is None else args.filter_bits


def _kmer_kw(args, command):
    """The k-mer keywords of the library call `command` makes: k, min_count, slots, prefilter and filter_bits always; of the
    other options the command takes those that were given (a flag that is on, a value, -F other than 0) and the row's `always`
    -- without an option the call is the one it was before the option existed.  With --kmers-from k is the set's unless -k
    names it: k=None."""
    row = _COMMANDS[command]
    kw = dict(k=_k(args), min_count=args.min_count, slots=args.slots, prefilter=args.prefilter, filter_bits=_filter_bits(args))
    for dest in row['options']:
        if dest in ('kmer', 'min_count', 'slots', 'prefilter', 'filter_bits'):
            continue
        value = getattr(args, dest)
        if dest in row.get('always', ()) or not (value is None or value == 0):
            kw[dest] = value
    if 'kmers_from' in kw:
        kw['k'] = args.kmer
    return kw


def _start(join=True):
    """Before a command's first device work: join the process group if a launcher started this process (torch, RCCL; not
    `count`, which never joins one); else, on one GPU with torch not imported and KBBQ_USE_TORCH unset, device memory,
    page-locked slabs, copies and events come from the library's own C ABI (kbbq/_hipmem.py) and `import torch` (~1 s with
    its HIP context) never happens.  True in that case."""
    import os
    import sys
    world = 1
    if join:
        from . import parallel
        world, _ = parallel.init_from_env()      # one process per GPU under torch.distributed.run; no-op otherwise
    if world > 1 or 'torch' in sys.modules or os.environ.get('KBBQ_USE_TORCH'):
        return False
    from . import _device
    _device.use_native_memory()
    return True


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


_BAM_INDEX_HELP = ('With --bam-out and -o FILE: write the index of the BAM file beside it in the same pass, reduced on the GPU while '
                   'the records are assembled: FILE.bai (bai), FILE.csi (csi: for references over 2^29 = 512 Mbp, which a BAI cannot '
                   'index), or whichever the @SQ lines call for (auto, the default of a bare --bam-index).  The alignments must be '
                   'in coordinate order; an existing index is overwritten.')


def _bam_out_kw(args):
    """{'bam_out': True} with --bam-out and {'bam_index': KIND} with --bam-index, else {}: without an option every call is the
    one it was."""
    kw = {'bam_out': True} if getattr(args, 'bam_out', False) else {}
    if getattr(args, 'bam_index', None) is not None:
        kw['bam_index'] = args.bam_index
    return kw


def _refuse_bam_out_ranks(args):
    """--bam-out under a launcher: refused before the process group is joined."""
    from . import parallel
    if getattr(args, 'bam_out', False) and parallel.launched_from_env():
        from .gatk.applybqsr import BAM_OUT_RANKS
        raise ValueError(BAM_OUT_RANKS)


def _recalibrate_bam_kmers(args):
    """`recalibrate -b ALN --kmers`: `bqsr --kmers` and `applybqsr` in one run (kbbq/recalibrate.py recalibrate_bam)."""
    import sys
    from . import kmer
    kmers = _kmer_kw(args, 'recalibrate')
    records = {key: kmers[key] for key in ('mixed_lengths', 'exclude_flags') if key in kmers}
    # every rank of a launcher refuses here, before it joins the process group
    _refuse_bam_out_ranks(args)
    _recal.check_bam_kmers(args.bam, args.gatkreport, args.output, kmers['k'], kmers['min_count'], kmers['prefilter'],
                           kmers['filter_bits'], **{key: kmers[key] for key in ('partitions', 'passes', 'exclude_flags', 'kmers_from')
                                                    if key in kmers}, **_bam_out_kw(args))
    from . import aln
    from ._trace import stage
    with stage('[recalibrate_bam, wall]'):
        with stage('parse'):
            # the one parse; what the records are refused for, before the device is touched -- but with --bam-out and
            # KBBQ_GPU_BAM=1, where a BAM file's records are decoded there and stay for the writer (kbbq/_bamin.py)
            bam = aln.alignments(args.bam, device=None if getattr(args, 'bam_out', False) else False, keep_stream=True)
        _recal.check_bam_records(bam, args.use_oq, _k(args), kmers['min_count'], kmers['prefilter'], kmers['filter_bits'], **records)
        _start()                                 # no process group: check_bam_kmers has refused a launcher's ranks
        info = _recal.recalibrate_bam(bam, use_oq=args.use_oq, set_oq=args.set_oq, kmers=kmers, gatkreport=args.gatkreport,
                                      output=args.output, **args.quantize, **_bgzf_kw(args), **_bam_out_kw(args))
    sys.stderr.write(kmer.summary_line('recalibrate', info, kmers, 'flagged_bases'))


def recalibrate(args):
    import os
    if args.kmers:
        return _recalibrate_bam_kmers(args)
    kopts = None
    if args.correct is not None:
        kopts = _kmer_kw(args, 'recalibrate')
        # every rank of a launcher refuses here, before it joins the process group
        _recal.check_corrected(args.correct, args.gatkreport, _k(args), kopts['min_count'], kopts['prefilter'], kopts['filter_bits'],
                               **{key: kopts[key] for key in ('partitions',) if key in kopts})
    if _start() and _ENDS_WITH_THE_COMMAND and not os.environ.get('KBBQ_SLOW_EXIT'):
        # this process ends right after its last byte (_leave): what it holds goes with it instead of being returned piece by piece
        from . import _hipmem, fastx
        _hipmem.cuda.keep_released_memory(True)
        fastx.LEAVE_OPEN = True
    if kopts is not None:
        import sys
        from ._trace import stage
        with stage('[recalibrate_corrected, wall]'):
            info = _recal.recalibrate_corrected(args.correct, infer_rg=args.infer_rg, gatkreport=args.gatkreport, output=args.output,
                                                **kopts, **args.quantize, **_bgzf_kw(args))
        from .kmer import summary_line
        sys.stderr.write(summary_line('recalibrate', info, kopts))
        return
    _recal.recalibrate(bam=args.bam, fastq=args.fastq, infer_rg=args.infer_rg,
                       use_oq=args.use_oq, set_oq=args.set_oq, gatkreport=args.gatkreport, output=args.output, **args.quantize,
                       **_bgzf_kw(args))


def benchmark(args):
    from . import benchmark as _bm
    from . import parallel
    parallel.init_from_env()          # one process per GPU under torch.distributed.run; no-op otherwise
    kmers = dict(kmers=_kmer_kw(args, 'benchmark')) if args.kmers else {}      # without the flag the call is what it was
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
        import sys
        from . import kmer
        _start()                             # under a launcher every rank joins its group, and bam_to_kmer_covariates refuses on each
        info = {}
        more = _kmer_kw(args, 'bqsr')
        # (KBBQ_GPU_BAM=1: a BAM file's records are decoded on the device, kbbq/_bamin.py; without it this IS AlignmentFile(args.bam))
        bam = aln.alignments(args.bam, planes=('seq', 'oq' if args.use_oq else 'qual'))
        _bqsr.bam_to_report_kmers(bam, use_oq=args.use_oq, info=info, **more).write(args.gatkreport)
        sys.stderr.write(kmer.summary_line('bqsr', info, more, 'flagged_bases'))
        return
    from . import benchmark as _bm
    _bqsr.bam_to_report(aln.AlignmentFile(args.bam), args.reference, _bm.get_var_sites(args.vcf)).write(args.gatkreport)


def correct(args):
    import os
    import sys
    if 'RANK' not in os.environ and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        sys.exit('kbbq correct: WORLD_SIZE > 1 but no RANK: start one process per GPU with torch.distributed.run, or run '
                 'it on one GPU without WORLD_SIZE')
    _start()
    from . import kmer
    kmer.main_correct(args.fastq, output=args.output, **_kmer_kw(args, 'correct'), **_bgzf_kw(args))


def count(args):
    from . import kmerset
    opts = dict(k=args.kmer, keep=args.keep, slots=args.slots, prefilter=args.prefilter, filter_bits=_filter_bits(args),
                partitions=1 if args.partitions is None else args.partitions,
                kmer_min_qual=args.kmer_min_qual, use_oq=args.use_oq, exclude_flags=args.exclude_flags or 0, histo=args.histo)
    # every rank of a launcher refuses here, before it joins a process group, and everything else count refuses on its arguments
    kmerset.check_count(args.fastq, args.bam, args.output, opts['k'], opts['keep'], opts['prefilter'], opts['filter_bits'],
                        opts['partitions'], opts['kmer_min_qual'], opts['use_oq'], opts['exclude_flags'])
    _start(join=False)                       # check_count has refused a launcher's ranks
    kmerset.main_count(args.fastq, args.bam, args.output, **opts)


def build_parser():
    """The parser and its sub-parsers by command name."""
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
    _add_kmer_options(rp, 'recalibrate')
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
    rp.add_argument('--bam-index', nargs='?', const='auto', default=None, choices=('auto', 'bai', 'csi'),
                    help='with -b --kmers: ' + _BAM_INDEX_HELP)
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
    _add_kmer_options(bp, 'benchmark')
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
    ap.add_argument('--bam-index', nargs='?', const='auto', default=None, choices=('auto', 'bai', 'csi'), help=_BAM_INDEX_HELP)
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
    _add_kmer_options(qp, 'bqsr', last='filter_bits')
    qp.add_argument('-u', '--use-oq', action='store_true', help='with --kmers: qualities from the OQ tag instead of QUAL')
    _add_kmer_options(qp, 'bqsr', first='skip_unresolved')
    qp.set_defaults(command=bqsr)

    cp = sub.add_parser('correct', description='Correct substitution errors of a FASTQ file with k-mer counts (GPU); the output '
                        'is the error-corrected file `recalibrate -f` takes')
    cp.add_argument('-f', '--fastq', required=True, help='FASTQ file to correct (plain or .gz)')
    _add_kmer_options(cp, 'correct', last='kmer_min_qual')
    cp.add_argument('-o', '--output', default=None,
                    help='Write the corrected FASTQ to this file instead of stdout; under torch.distributed.run every rank '
                         'writes FILE.rankNNNN, to be concatenated in rank order.')
    cp.add_argument('--bgzf', action='store_true', help=_BGZF_HELP)
    _add_kmer_options(cp, 'correct', first='kmers_from')
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
    _add_kmer_options(np_, 'count', last='kmer')
    np_.add_argument('--keep', type=int, default=2,
                     help='write the k-mers seen at least this often (default 2, the smallest threshold the histogram\'s valley can '
                          'give); a --min-count below it cannot be served from the set; >= 2 with --prefilter')
    _add_kmer_options(np_, 'count', first='slots', last='kmer_min_qual')
    np_.add_argument('-u', '--use-oq', action='store_true', help='with -b and --kmer-min-qual: gate by the OQ tag instead of QUAL')
    _add_kmer_options(np_, 'count', first='exclude_flags')
    np_.add_argument('--histo', default=None, metavar='FILE',
                     help='write the count histogram as `count<TAB>k-mers` lines for counts --keep..256 (the last line: 256 and more), '
                          'the shape Jellyfish prints and GenomeScope reads')
    np_.set_defaults(command=count)
    return parser, dict(recalibrate=rp, benchmark=bp, applybqsr=ap, bqsr=qp, correct=cp, count=np_)


def _validate(parsers, args):
    """What the parser refuses of a parsed command line, with exit status 2: decided here, before the device is touched and,
    under a launcher, before a process group could exist.  Sets args.quantize for the commands that apply a model."""
    name = args.command.__name__
    if name not in parsers:
        return
    parser, rows = parsers[name], _COMMANDS.get(name, {}).get('only_with', ())
    flag = {action.dest: '/'.join(action.option_strings) for action in parser._actions}

    def given(dests):
        values = ((dest, getattr(args, dest, None)) for dest in dests)
        return [flag[dest] for dest, value in values if value is not None and value is not False]     # -F 0 is given

    def only_with(rows):
        for dests, mode, words in rows:
            if given(dests) and not mode(args):
                parser.error('%s: only with %s' % (', '.join(given(dests)), words))

    if given(('kmers_from',)):
        only_with(row for row in rows if row[0] == ('kmers_from',))
        if given(_COUNTING_OPTIONS):
            parser.error('%s: not with --kmers-from (counting options: the k-mers come counted)' % ', '.join(given(_COUNTING_OPTIONS)))
    if name == 'count':
        if not args.fastq and not args.bam:
            parser.error('at least one input is required: -f FASTQ [FASTQ ...] and / or -b ALN [ALN ...]')
        if args.output is None:
            parser.error('the following arguments are required: -o/--output')
    if name in ('recalibrate', 'applybqsr'):
        args.quantize = _quantize(parser, args)
        if args.bam_out and args.bgzf:
            parser.error('--bam-out: not with --bgzf (a BAM file is a BGZF file already)')
    only_with(rows)
    if name in ('recalibrate', 'applybqsr') and args.bam_index is not None:
        if not args.bam_out:
            parser.error('--bam-index: only with --bam-out (it indexes the BAM file that option writes)')
        if args.output is None:
            parser.error('--bam-index: needs -o FILE (an index of stdout has no name; it is written to FILE.bai or FILE.csi)')
    if name == 'recalibrate' and args.kmers and given(('fix_n', 'infer_rg')):
        parser.error('%s: not with -b --kmers (FASTQ input only)' % ', '.join(given(('fix_n', 'infer_rg'))))
    if name == 'benchmark' and args.kmers and args.fastq is not None:
        parser.error('-f/--fastq: not with --kmers (the k-mers are those of the alignments\' own sequences)')
    if name == 'bqsr':
        if args.kmers and given(('reference', 'vcf')):
            parser.error('%s: not with --kmers (its errors come from the alignments\' own k-mers)' % ', '.join(given(('reference', 'vcf'))))
        missing = [flag[dest] for dest in ('reference', 'vcf') if getattr(args, dest) is None]
        if not args.kmers and missing:
            parser.error('the following arguments are required: %s' % ', '.join(missing))


def main(argv=None):
    parser, parsers = build_parser()
    args = parser.parse_args(argv)
    _validate(parsers, args)
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
