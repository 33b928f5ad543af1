"""
kbbq.recalibrate -- drop-in for the reference module of the same name
(reference kbbq/recalibrate.py:13-174), with both per-read Python loops replaced
by HIP kernels on an MI355X:

    pass 1  fastq_to_covariate_arrays  -> K1 (error flagging + covariate binning)
    model   applybqsr.get_delta_qs     -> host, same SciPy call as the reference
    pass 2  recalibrate_fastq          -> K2 (delta-Q LUT apply), FASTQ text to stdout

Behaviour kept: argument names and defaults, the 9-tuple order, int64 arrays
owned by the caller, output through print(), and the exceptions the reference
raises on bad input (AssertionError, IndexError, TypeError, NotImplementedError,
ValueError -- SURVEY.md 8(b)).

Deliberate deviations (also in README.md / INTEGRATION.md):
  * gatkreport: the reference raises NotImplementedError for ANY value (recalibrate.py:167-168); here `-g FILE` with FASTQ
    input saves / loads the model; without FASTQ input it raises NotImplementedError as the reference.
  * maxscore: the device tables have the reference's default Q axis (43 = maxscore 42 + 1); another maxscore raises
    ValueError instead of being honoured.
  * output=...: an extra keyword (the reference only prints): write to a file, one file per rank under torch.distributed.
"""
import os

import numpy as np

from . import compare_reads as utils        # noqa: F401  (module attribute of the reference: recalibrate.utils)
from . import fastx
from . import _bgzf
from . import _device as dev
from . import _solve
from . import _stream
from . import parallel
from ._trace import stage
from .gatk import applybqsr


def find_corrected_sites(uncorr_read, corr_read):
    """Boolean array, True where the corrected sequence differs from the original."""
    assert corr_read.name.startswith(uncorr_read.name)
    a = np.frombuffer(uncorr_read.sequence.encode('utf-32-le'), dtype=np.uint32)
    b = np.frombuffer(corr_read.sequence.encode('utf-32-le'), dtype=np.uint32)
    if a.shape != b.shape:
        raise ValueError('operands could not be broadcast together with shapes %s %s' % (a.shape, b.shape))
    return a != b


def _vectors_from_tables(pos_errs, pos_total, dinuc_errs, dinuc_total, maxscore):
    return _solve.vectors_from_tables(pos_errs, pos_total, dinuc_errs, dinuc_total, maxscore)


LAST_RUN = {}            # what the most recent recalibrate_fastq did per length band (layouts, bytes uploaded): bench.py, traces


def _tally_local(packed, minscore, maxscore, band_rows=fastx.band_rows):
    """K1 over this rank's packed reads, length band by length band -> device Tables (zero tables when the rank has
    no reads).  Each band is tallied in the layout the packer wrote it in (fastx._fill_bands); whatever that path reports
    (bad input, a shape it does not serve) is redone one read per row, which carries the reference's exact error semantics.  The read index
    of a kernel-reported error is made relative to the rank's first read.  band_rows: what makes a band's one-read-per-row
    batch for that redoing (recalibrate_corrected: fastx.band_rows, then the corrected plane from the k-mer table)."""
    if maxscore != 42:
        raise ValueError('the Q axis of the device tables is fixed at 43 (maxscore = 42)')
    R, S = max(packed['R'], 0), packed['S']
    if R == 0 or S == 0:
        return None
    if packed.get('streamed'):
        # a shard larger than the device budget: nothing is resident, the reads go through K1 slab by slab (kbbq/_stream.py)
        st = packed['streamed']
        st['peak'] = _stream.Peak(st['budget'])
        tables = dev.Tables(R, 2 * S)
        _stream.tally_range(st['A'], st['B'], st['infer_rg'], st['lo'], st['hi'], tables, minscore, st['budget'])
        return tables
    tables = dev.Tables(R, 2 * S)

    def tally_band(band, laid):
        hints = dict(s_band=band['S'], s_min=band.get('Smin', 0))
        if laid is not None:
            part = dev.Tables(R, 2 * S)
            try:
                dev.accumulate(laid, part, minscore, **hints)
                tables.add(part)
                band['laid'] = laid
                return
            except (IndexError, TypeError, ValueError, dev.N.LutNeedsCheckedApply):
                band['laid'] = None          # bad input or an unsupported shape: the row-per-read kernel decides
        dev.accumulate(band_rows(band), tables, minscore, **hints)

    # several length bands (a mixed-length input, BASELINE config 5): ONE launch over all of them, each band on its share of
    # the workgroups (kbbq_accumulate_bands_dev); whatever any band's kernel reports sends them all band by band below, where
    # each has its own fallback and the first offending read is found
    done = set()
    several = [b for b in packed['bands'] if 'source' in b and b.get('laid') is not None]
    if len(several) >= 2:
        part = dev.Tables(R, 2 * S)
        try:
            with stage('K1', sync=True):
                dev.accumulate_bands([(b['laid'], b['S'], b.get('Smin', 0)) for b in several], part, minscore)
            tables.add(part)
            done = {id(b) for b in several}
        except (IndexError, TypeError, ValueError, dev.N.LutNeedsCheckedApply):
            pass
    for band in packed['bands']:
        if id(band) in done:
            continue
        if 'source' in band:
            laid = band.get('laid')                    # written by the packer in its layout (fastx._fill_bands): nothing to convert
        else:                                          # host planes of a caller's own: tallied and applied as they are -- a
            with stage('H2D', sync=True):              # device pass into another layout costs more than it saves for ONE
                band['batch'] = dev.ReadBatch.from_host(band['seq'], band['qual'], band['meta'], cseq=band['cseq'])   # accumulate + apply
            laid = None
        band['laid'] = None                            # still resident: pass 2 re-uses them when it covers file A
        try:
            with stage('K1', sync=True):
                tally_band(band, laid)
        except (IndexError, TypeError) as e:
            if hasattr(e, 'read_index'):
                e.read_index = band['first'] + max(e.read_index, 0)
            raise
    return tables


def _tally(packed, minscore, maxscore):
    """_tally_local on every rank, agreement on the first error any rank's kernel reported (all ranks
    raise it), then ONE sum-allreduce of the count tables (RCCL over xGMI)."""
    exc, tables = None, None
    try:
        tables = _tally_local(packed, minscore, maxscore)
    except Exception as e:                   # noqa: BLE001 -- whatever stops one rank (bad input, a device error, out of
        exc = e                              # memory) must stop them all before anybody waits in the allreduce
    parallel.raise_first_error(exc, None if exc is None else packed.get('first', 0) + max(getattr(exc, 'read_index', 0), 0))
    if tables is not None:
        parallel.allreduce_tables(tables.buf)
    return tables


def _warm_up():
    """The process's one-time device costs (dev.warm_up), paid while the C++ reader works on the input files."""
    import sys
    torch = dev._backend or sys.modules.get('torch')         # the device this process selected (parallel.init_from_env), else 0
    device = torch.cuda.current_device() if torch is not None and torch.cuda.is_available() else 0
    with stage('warm-up'):
        dev.warm_up(device)


def _scan(path_a, path_b, infer_rg):
    """fastx.PairScan, started before the device warms up -- unless the reader is to inflate the input on the device
    (KBBQ_GPU_INFLATE=1 and a compressed file above the threshold): that needs the context, so the warm-up comes first."""
    from . import _bgzf
    if _bgzf.wants_device(path_a, path_b):
        _warm_up()
    return fastx.PairScan(path_a, path_b, infer_rg)


def _pack_and_tally(fastq, infer_rg, minscore, maxscore):
    world, rank = parallel.world_rank()
    # rank 0 (or the only process) opens and scans the pair on the reader's own threads -- no interpreter lock needed --
    # while the device warms up; the other ranks then index only the byte ranges of their shards (fastx.pack_pair)
    # (several ranks: every rank cuts, indexes and scans its own byte range of either file -- fastx.local_ranges -- and
    # only when the files do not cut alike does rank 0 scan all of them for a plan)
    scan = _scan(fastq[0], fastq[1], infer_rg) if world == 1 else None
    _warm_up()
    failure, packed = None, None
    try:
        packed = fastx.pack_pair(fastq[0], fastq[1], infer_rg, shard=(rank, world) if world > 1 else None, bands=True,
                                 scan=scan, to_device=True, exchange=parallel.broadcast_object if world > 1 else None,
                                 gather=parallel.all_gather_object if world > 1 else None, budget=dev.device_budget())
    except Exception as e:                   # noqa: BLE001 -- one rank's failure (its shard unreadable, out of memory) stops them all
        failure = e
    parallel.raise_first_error(failure, 0)
    err = packed.get('pending_error')
    if err is not None:
        # the reference fails at the FIRST offending read: let the kernel look at the reads
        # before it (and at it, when its own checks come first) before raising the host error
        idx, exc, inclusive = err
        try:
            _tally(packed, minscore, maxscore)
        finally:
            if packed.get('other') is not None:
                fastx.close_later(packed.pop('other'))
        raise exc
    try:
        tables = _tally(packed, minscore, maxscore)
    finally:
        # the corrected file is not needed past the tally.  It is only RETIRED here (no new work starts on it) and unmapped by the
        # caller after its last byte: unmapping 2.5 GB holds the address space's lock for 30-40 ms, and done beside pass 2 --
        # as rounds 3 and 4 did -- it stalled the first slabs' page faults, buffer allocations and write(2) for as long
        if packed.get('other') is not None:
            packed['retired'] = fastx.retire(packed.pop('other'))
    if tables is not None and packed.get('total', packed['n']) == 0:
        tables = None
    return packed, tables


def fastq_to_covariate_arrays(fastq, infer_rg=False, minscore=6, maxscore=42):
    """Tally errors and observations of the (uncorrected, corrected) FASTQ pair by read
    group, reported quality, cycle and dinucleotide.  Returns the reference's 9-tuple:
    meanq, rg_errs, rg_total, q_errs, q_total, pos_errs, pos_total, dinuc_errs, dinuc_total."""
    if any(fastx.is_sequential_input(p) for p in fastq) or os.environ.get('KBBQ_SEQUENTIAL'):
        if maxscore != 42:
            raise ValueError('the Q axis of the device tables is fixed at 43 (maxscore = 42)')
        run = _Sequential(fastq, infer_rg)
        try:
            _warm_up()
            tables = run.pass1(minscore, spool=False)
        finally:
            run.close()
        packed = dict(R=len(run.rgs) if run.usable else 0, S=run.longest)
    else:
        packed, tables = _pack_and_tally(fastq, infer_rg, minscore, maxscore)
        if packed.get('retired') is not None:
            fastx.close_later(packed.pop('retired'))
    if tables is None:
        z = lambda *s: np.zeros(s, dtype=np.int64)
        R, S = packed['R'], packed['S']
        return _vectors_from_tables(z(R, 43, 2 * S), z(R, 43, 2 * S), z(R, 43, 16), z(R, 43, 16), maxscore)
    return _vectors_from_tables(*tables.to_host(), maxscore)


def _rg_order(rg_to_int):
    """Read-group names in id order, as text (the report's ReadGroup column)."""
    return [str(k) for k, _ in sorted(rg_to_int.items(), key=lambda kv: kv[1])]


def save_model(tables, rg_to_int, path):
    """Count tables (K1 output) -> GATK recalibration report file (gatk/bqsr.py
    vectors_to_report; the option main.py:55-58 declares)."""
    from .gatk import bqsr
    vectors = _vectors_from_tables(*tables.to_host(), 42)
    bqsr.vectors_to_report(*vectors, _rg_order(rg_to_int)).write(path)


def load_model(path, rg_to_int):
    """GATK recalibration report file -> device count tables for the given read groups
    (gatk/applybqsr.py table_to_vectors).  meanq is NOT taken from the 4-decimal
    EstimatedQReported column: K3 recomputes it from the counts exactly as pass 1 would have,
    so a saved-and-reloaded model recalibrates identically to a fresh one."""
    from . import recaltable
    report = recaltable.RecalibrationReport.fromfile(path)
    vectors = applybqsr.table_to_vectors(report, _rg_order(rg_to_int))
    return dev.Tables.from_host(*vectors[5:9])


def _collective(fn, first=0):
    """fn() on every rank; if a kernel of any rank flagged bad input, all ranks raise the error of the
    globally first offending read (a single process would have stopped there)."""
    exc, res = None, None
    try:
        res = fn()
    except Exception as e:                   # noqa: BLE001 -- see _tally
        exc = e
    parallel.raise_first_error(exc, None if exc is None else first + max(getattr(exc, 'read_index', 0), 0))
    return res


def _device_qmap(quantize):
    """The checked 256-byte map of `quantize` on the device (dev.qmap_to_device), or None: what every apply site carries beside
    `lut, shape`."""
    return None if quantize is None else dev.qmap_to_device(quantize)


@_bgzf.option
def recalibrate_fastq(fastq, infer_rg=False, gatkreport=None, output=None, quantize=None):
    """Recalibrate FASTQ file fastq[0] using its error-corrected version fastq[1];
    the recalibrated FASTQ is printed to stdout.  K1 -> K3 -> K2, tables and LUT stay on
    the device between the kernels.  gatkreport (the reference declares the option and raises
    NotImplementedError, recalibrate.py:167-168): an existing report replaces pass 1 (fastq[1]
    is not read); otherwise the model of pass 1 is saved there.
    Under torch.distributed (one process per GPU, parallel.init_from_env) every rank takes a contiguous
    shard of the records, the count tables are summed with one allreduce, the solve is replicated and
    the ranks print their records in rank order: the concatenated output is the single-process output.
    output (not in the reference, which only prints): write the records to this file instead of stdout; with several
    ranks every rank writes ITS records to `output`.rankNNNN at the same time (the files, concatenated in rank order,
    are the single-process output) -- ranks sharing one stdout can only write in turn.
    quantize (not in the reference): the 256-byte map of gatk.applybqsr.quantize_map (--static-quantized-quals); every quality
    plane K2 writes goes through it on the device before it is copied back.  Per byte: the model, the report and the rank files'
    concatenation are what they are without it."""
    quantize = applybqsr._check_qmap(quantize)
    world, rank = parallel.world_rank()
    if any(fastx.is_sequential_input(p) for p in fastq) or os.environ.get('KBBQ_SEQUENTIAL'):
        return _recalibrate_sequential(fastq, infer_rg, gatkreport, output, quantize)
    shard = (rank, world) if world > 1 else None
    done_with = []                           # readers to unmap on a helper thread once the last byte is out (or the call has failed)
    try:
        return _recalibrate_mapped(fastq, infer_rg, gatkreport, output, world, rank, shard, done_with, quantize)
    finally:
        for reader in done_with:
            if reader is not None:
                fastx.close_later(reader)


def _recalibrate_mapped(fastq, infer_rg, gatkreport, output, world, rank, shard, done_with, quantize=None):
    """recalibrate_fastq on mapped, indexed inputs (regular files): resident on the device, or slab by slab within the budget."""
    packed, single = None, None
    if gatkreport is not None and os.path.exists(gatkreport):
        scan = _scan(fastq[0], None, infer_rg)
        _warm_up()
        text = scan.result()[0]
        done_with.append(text)
        if text.n == 0:
            return
        single = fastx.pack_single(text, infer_rg, shard, bands=True, to_device=True, budget=dev.device_budget())
        tables = load_model(gatkreport, single['rg_to_int'])
    else:
        packed, tables = _pack_and_tally(fastq, infer_rg, 6, 42)
        text = packed['text']
        done_with.extend([text, packed.get('retired')])
        if text.total == 0:
            return
        if tables is None:
            raise IndexError('index 0 is out of bounds for axis 0 with size 0')   # no read was tallied
        if gatkreport is not None:
            if rank == 0:
                save_model(tables, packed['rg_to_int'], gatkreport)
            parallel.barrier()
    with stage('solve', sync=True):
        lut, shape = dev.solve_lut(tables)
        qmap = _device_qmap(quantize)
    if packed is not None and packed['total'] == text.total:
        # pass 2 walks the same reads with the same first-appearance read groups (:141-148):
        # the planes of pass 1 are still on the device
        single = packed
    else:
        # file B was shorter (zip truncation), or the model came from a report: pass 2 covers
        # all of file A with its own first-appearance read groups
        if single is None:
            if text.n != text.total:
                text = fastx.NativeFastq(fastq[0])                 # a shard's reader: pass 2 needs all of file A
                done_with.append(text)
            single = fastx.pack_single(text, infer_rg, shard, bands=True, to_device=True, budget=dev.device_budget())

    if single.get('streamed'):
        return _emit_streamed(text, single, lut, shape, output, world, rank, qmap)
    _apply_and_emit(text, single, lut, shape, output, world, rank, qmap)


def _apply_and_emit(text, single, lut, shape, output, world, rank, qmap=None):
    """Pass 2 over resident bands: K2 on every band of `single` in its layout, then the records of `text` to stdout or `output`.
    qmap: the device map of static quantized qualities (dev.apply / dev.apply_bands)."""
    R = shape[0]
    if single['R'] != R:
        # pass 2 met read groups the model does not have (recalibrate.py:143-151: an IndexError at the first such read) or
        # fewer than it has: rows gathered by THEIR read-group segments do not fit the model's -- one read per row decides
        for band in single['bands']:
            band['laid'] = None

    def apply_band(band):
        return _stream.apply_band(band, lut, shape, qmap)

    def apply_shard():
        merged = {}
        several = [b for b in single['bands'] if b.get('laid') is not None]
        if len(several) >= 2:                 # all length bands in one launch (kbbq_apply_bands_dev); any trouble: band by band
            try:
                res = dev.apply_bands([(b['laid'], b['S'], b.get('Smin', 0)) for b in several], lut, shape, restore_order=True,
                                      qmap=qmap)
                for b, o in zip(several, res):
                    merged[id(b)] = o
                    two = isinstance(b['laid'], dev.PairBatch)
                    b['out_flags'], b['out_S2'] = (dev.N.ROWS_PAIRS, 2 * b['laid'].S) if two else (0, 0)
            except (IndexError, TypeError, ValueError, dev.N.LutNeedsCheckedApply):
                merged = {}
        outs = []
        for band in single['bands']:
            if id(band) in merged:
                outs.append(merged[id(band)])
                continue
            try:
                outs.append(apply_band(band))
            except (IndexError, TypeError, ValueError) as e:
                if hasattr(e, 'read_index'):
                    e.read_index = band['first'] + max(e.read_index, 0)
                raise
        return outs
    with stage('apply', sync=True):
        outs = _collective(apply_shard, single['first'])
    LAST_RUN.clear()
    LAST_RUN['bands'] = [dict(reads=b['n'], longest=b['S'],
                              layout=(b['laid'] if b.get('laid') is not None else b['batch']).describe(),
                              written_by='the FASTQ packer (kbbq_fastq_fill_rows)' if b.get('laid') is not None and 'source' in b else
                                         'the row-per-read packer (kbbq_fastq_fill_range)',
                              h2d_bytes=sum(getattr(x, 'h2d_bytes', 0) for x in (b.get('laid'), b.get('batch')) if x is not None),
                              output_rows='mate-pair rows, read by the writer as they are' if b.get('out_flags') else 'one read per row')
                         for b in single['bands']]

    # recalibrate.py:153-156: '@' + name, sequence, '+', qualities
    from . import _egress
    if output is None and _bgzf.enabled():
        def compressed():
            with _bgzf.stdout_sink() as sink:
                _egress.emit_records(text, single['first'], single['bands'], outs, sink=sink)
        parallel.in_rank_order(compressed)
    elif output is None:
        parallel.in_rank_order(lambda: _egress.emit_records(text, single['first'], single['bands'], outs))
    else:
        with _bgzf.open_sink(output if world == 1 else '%s.rank%04d' % (output, rank)) as sink:
            _egress.emit_records(text, single['first'], single['bands'], outs, sink=sink)


TWO_COMMANDS = ('run the two commands instead: `kbbq correct -f reads.fq -o reads.cor.fq`, then '
                '`kbbq recalibrate -f reads.fq reads.cor.fq`')


def check_corrected(path, gatkreport=None, k=31, min_count=None, prefilter=False, filter_bits=4, partitions=1):
    """What recalibrate_corrected refuses, before any device work and, under a launcher, before the process group exists."""
    from . import kmer
    kmer._check_partitions(partitions, launched=parallel.launched_from_env())
    if not 8 <= int(k) <= 32:
        raise ValueError('k must be in 8..32, got %d' % int(k))
    if min_count is not None and int(min_count) < 1:
        raise ValueError('min_count must be >= 1, got %d' % int(min_count))
    if parallel.launched_from_env() or kmer._ranks() is not None:
        raise ValueError('recalibrate -c does not run across ranks yet (every rank would need the k-mers of all reads): '
                         'on one GPU, or ' + TWO_COMMANDS + ', both of which run under a launcher')
    if prefilter:
        kmer._check_prefilter(min_count, filter_bits)
    if fastx.is_sequential_input(path) or os.environ.get('KBBQ_SEQUENTIAL'):
        raise ValueError('recalibrate -c keeps the reads on the device between correction and recalibration and takes inputs '
                         'that can be mapped only (not pipes, standard input, KBBQ_SEQUENTIAL or .gz files of '
                         'KBBQ_GZ_STREAM_BYTES and more): ' + TWO_COMMANDS)
    if gatkreport is not None and os.path.exists(gatkreport):
        raise ValueError('the report %s exists: its model replaces pass 1, so there is nothing to correct the reads for; '
                         'give -f with the report, or the name of a report to write' % gatkreport)


@_bgzf.option
def recalibrate_corrected(path, infer_rg=False, gatkreport=None, output=None, k=31, min_count=None, slots=None, prefilter=False,
                          filter_bits=4, fix_n=False, passes=1, skip_unresolved=False, partitions=1, quantize=None,
                          kmer_min_qual=None, kmers_from=None):
    """`kbbq correct` and `kbbq recalibrate -f reads corrected` in one run over ONE file: the reads go to the device once, in
    the layout pass 2 uses (fastx.pack_single), their k-mers are counted and the reads corrected where they lie
    (kmer.count_batch / correct_batch: the corrected plane is each band's cseq), and the tally, the solve, the apply and the
    writer run over the same resident planes.  Nothing is written or read between correction and recalibration.  The output
    is, byte for byte, that of the two commands.  Returns info: k, min_count, hist, reads, changed_bases, slots (and
    admitted with the prefilter) and fix_n.  fix_n: the N rule of `kbbq correct --fix-n` in every band's own layout -- a fixed N
    reaches K1 as the difference from the original's N it is in the two-file form.  gatkreport: the model of the tally is saved there; an existing report is refused.
    passes: `kbbq correct --passes P` in every band's own layout (kmer.correct_batch); info carries it.
    skip_unresolved: a base the k-mers contradict without naming a replacement (untrusted, and no substitution wins) is left out of
    the tally, neither error nor observation, instead of counting as correct.  Every band gets a tally plane beside its corrected
    plane -- its qualities with byte 0 at those bases (kbbq_kmer_correct_rows_skip_dev) -- which K1 reads in the place of the
    qualities; K1 drops a base of quality below minscore by the base's own byte, so nothing changes for the neighbours.  The
    solve, K2 and the writer see the qualities as read; the planes (one n x pitch per band) are released before the apply.
    info['skipped_bases']: the unresolved bases of all reads.  The output is that of `recalibrate -f reads corrected` with the
    model tallied from a reads file whose unresolved bases have quality '!'.
    partitions: `kbbq correct --partitions` (kmer.count_block): every round counts every band's rows for one partition of the
    k-mers through a table of `slots` slots (default: kmer.partition_slots within what the budget leaves beside the reads), and
    the table kept until the tally is over is the solid table, against which the bands -- those redone as character rows too --
    are corrected.  The same bytes; info then carries partitions, kept_pairs and solid_slots, and slots is the per-partition table.
    quantize: recalibrate_fastq's -- the written qualities only; the correction, the tally and the model do not see it.
    kmer_min_qual: `kbbq correct --kmer-min-qual Q` (kmer.gate_batch): every band is gated by its own quality plane, in its own
    layout, into one word of counted windows; the prefilter, the count and every partition round read the gated planes, which
    are held until the count is over (one sequence plane per band) and size the filter and the default table; the bands are
    corrected and tallied as read.  info then carries kmer_min_qual, counted_windows and windows.
    kmers_from: a k-mer set file (kmer.load_set) in the place of the prefilter, the count, the histogram and the threshold: the
    table is loaded within what the budget leaves beside the reads, k is the set's (pass k=None, or the set's), no counting
    option goes with it, and everything after is what it is.  info then carries kmers_from and loaded_kmers.
    One process, mapped inputs, reads that fit the device budget: anything else raises ValueError naming the two commands."""
    from . import kmer
    quantize = applybqsr._check_qmap(quantize)
    passes = kmer.check_passes(passes)
    kmers_from = kmer.check_kmers_from(kmers_from, prefilter, filter_bits, partitions, kmer_min_qual)
    kmer_min_qual = kmer.check_kmer_min_qual(kmer_min_qual)
    if kmers_from is not None:
        k = kmer.set_k(kmers_from, k)                # the header alone: no device
    check_corrected(path, gatkreport, k, min_count, prefilter, filter_bits, **kmer._partitions_kw(partitions))
    done_with = []
    try:
        return _recalibrate_corrected(path, infer_rg, gatkreport, output, int(k), min_count, slots, prefilter, filter_bits, done_with,
                                      bool(fix_n), passes, bool(skip_unresolved), partitions, quantize,
                                      **kmer._min_qual_kw(kmer_min_qual), **kmer._kmers_from_kw(kmers_from))
    finally:
        for reader in done_with:
            fastx.close_later(reader)


def _batch_bytes(batch):
    return sum(int(x.numel()) * int(x.element_size()) for x in (batch.seq, batch.cseq, batch.qual, batch.meta,
                                                               getattr(batch, 'out_plane', None)) if x is not None)


def _recalibrate_corrected(path, infer_rg, gatkreport, output, k, min_count, slots, prefilter, filter_bits, done_with, fix_n=False,
                           passes=1, skip=False, partitions=1, quantize=None, kmer_min_qual=None, kmers_from=None):
    from . import kmer
    more = kmer._passes_kw(passes)
    if skip:
        more['skip_unresolved'] = True
    scan = _scan(path, None, infer_rg)
    _warm_up()
    text = scan.result()[0]
    done_with.append(text)
    info = dict(k=k, min_count=int(min_count or 0), hist=np.zeros(kmer.HIST, dtype=np.int64), reads=int(text.n), changed_bases=0,
                slots=0, fix_n=fix_n, passes=passes)
    if skip:
        info['skipped_bases'] = 0
    if prefilter:
        info['admitted'] = 0
    if text.n == 0:
        return info
    budget = dev.device_budget()
    single = fastx.pack_single(text, infer_rg, None, bands=True, to_device=True, budget=budget)
    if single.get('streamed'):
        raise ValueError('%d reads of up to %d bases do not fit the device budget of %d bytes (KBBQ_DEVICE_BUDGET) and would be '
                         'streamed, but recalibrate -c corrects the reads where they lie: ' % (single['n'], single['S'], budget)
                         + TWO_COMMANDS)
    rows = [b['laid'] if b.get('laid') is not None else b['batch'] for b in single['bands']]
    windows = sum(kmer.batch_windows(r, k) for r in rows)
    # what the planes hold once every band has its corrected plane beside the others
    resident = sum(_batch_bytes(r) + (0 if r.cseq is not None else int(r.seq.numel())) for r in rows)
    # ... and room for the one-read-per-row planes (seq, cseq, qual, sidecar) of the largest band a layout's kernel may refuse,
    # which are made while the table is still there (corrected_rows below); pass 1 of `-f` redoes bands one at a time too
    # (with skip: the tally plane of every band, and of that band's character rows)
    if skip:
        resident += sum(int(r.qual.numel()) for r in rows)
    resident += max(int(b['n']) * ((4 if skip else 3) * int(b['pitch']) + 4) for b in single['bands'] if b.get('laid') is not None) \
        if any(b.get('laid') is not None for b in single['bands']) else 0
    table = None
    read_quals = []                   # skip: (batch, its qualities as read) while the tally plane stands in their place
    gated = [None] * len(rows)        # kmer_min_qual: the plane of each band the prefilter and the count read in the place of its seq
    if kmer_min_qual is not None:
        with stage('k-mer gate', sync=True):
            word = dev._torch().zeros(1, dtype=dev._torch().int64, device='cuda')
            for i, r in enumerate(rows):
                gated[i], counted = kmer.gate_batch(r, k, kmer_min_qual, windows=word)
            del word
        info.update(kmer_min_qual=kmer_min_qual, counted_windows=counted, windows=windows)
        windows = counted
        resident += sum(int(g.numel()) for g in gated)       # ... until the count is over

    def tally_plane(batch):
        read_quals.append((batch, batch.qual))
        batch.qual, batch.tally_qual = batch.tally_qual, None

    def read(what, **kw):
        for r, g in zip(rows, gated):
            (kmer.prefilter_batch if what == 'prefilter' else kmer.count_batch)(r, k, plane=g, **kw)
    try:
        try:
            table, hist, t, counting = kmer.count_block(read, windows, k, min_count=min_count, slots=slots, prefilter=prefilter,
                                                        filter_bits=filter_bits, partitions=partitions, kmers_from=kmers_from,
                                                        room=budget - resident, stage=stage)
        except (ValueError, dev.N.KmerTableFull) as exc:
            if 'slots' not in str(exc):
                raise
            raise type(exc)('%s -- the k-mer table shares the device budget (KBBQ_DEVICE_BUDGET) with %d bytes of resident reads: '
                            'give --slots, or --prefilter for a table several times smaller' % (exc, resident)) from None
        del gated[:]                                   # the count is over: everything below reads the bands as read
        info.update(hist=hist, min_count=t, slots=counting['slots'])
        if prefilter:
            info['admitted'] = counting['admitted']
        if counting.get('partitions', 1) > 1:
            info.update({key: counting[key] for key in ('partitions', 'table_bytes', 'kept_pairs', 'solid_slots')})
        if kmers_from is not None:
            info.update(kmers_from=counting['kmers_from'], loaded_kmers=counting['loaded_kmers'])
        with stage('k-mer correct', sync=True):
            for r in rows:
                counts = kmer.correct_batch(table, r, t, fix_n=fix_n, **more)
                if skip:
                    counts, unresolved = counts
                    info['skipped_bases'] += int(unresolved.cpu().numpy().astype(np.int64).sum())
                    tally_plane(r)
                info['changed_bases'] += int(counts.cpu().numpy().astype(np.int64).sum())

        def corrected_rows(band):
            # a band whose layout the tally refuses is redone one character row per read; its corrected characters come from the
            # character kernels on those rows, which is why the table lives until the tally is over (skip: its tally plane too)
            batch = fastx.band_rows(band)
            if batch.cseq is None:
                kmer.correct_batch(table, batch, t, fix_n=fix_n, **more)
                if skip:
                    tally_plane(batch)
            return batch
        tables = _tally_local(single, 6, 42, band_rows=corrected_rows)
    finally:
        for batch, qual in read_quals:                 # the solve, K2 and the writer see the qualities as read; the tally
            batch.qual = qual                          # planes are released here, before the apply
        if table is not None:
            table.close()
    if tables is None:
        raise IndexError('index 0 is out of bounds for axis 0 with size 0')   # no read was tallied
    if gatkreport is not None:
        save_model(tables, single['rg_to_int'], gatkreport)
    with stage('solve', sync=True):
        lut, shape = dev.solve_lut(tables)
    _apply_and_emit(text, single, lut, shape, output, 1, 0, _device_qmap(quantize))
    return info


def _prefetched(items, depth=1):
    """Iterate `items` (a generator whose steps spend their time in C calls that release the interpreter lock: reading and
    indexing the next segment of an input) on a helper thread, `depth` items ahead of the consumer."""
    import queue
    import threading
    q, end = queue.Queue(depth), object()
    stop = threading.Event()

    def run():
        try:
            for it in items:
                if stop.is_set():
                    break
                q.put((it, None))
        except BaseException as e:           # noqa: BLE001 -- re-raised by the consumer
            q.put((None, e))
            return
        q.put((end, None))
    th = threading.Thread(target=run, daemon=True)
    th.start()
    try:
        while True:
            it, exc = q.get()
            if exc is not None:
                raise exc
            if it is end:
                return
            yield it
    finally:
        stop.set()
        while th.is_alive():                 # let a producer blocked on the full queue see the stop
            try:
                q.get_nowait()
            except queue.Empty:
                th.join(0.01)


SEGMENT_BYTES = 256 << 20                    # text of file A per segment of a sequentially read input (KBBQ_SEGMENT_BYTES)


def _segment_bytes():
    env = os.environ.get('KBBQ_SEGMENT_BYTES')
    return max(dev.parse_bytes(env), 1 << 16) if env else SEGMENT_BYTES


def _pair_segments(sa, sb, seg_bytes):
    """(segment of file A, segment of file B holding the same number of records -- fewer, or None, once file B has ended)
    until file A ends; without sb: (segment of A, None)."""
    import threading
    b_ended = sb is None
    while True:
        ahead = None
        if not b_ended:                      # both inputs are drained at the same time (two pipes fed by two decompressors)
            ahead = threading.Thread(target=_quietly, args=(sb.prefetch, seg_bytes), daemon=True)
            ahead.start()
        try:
            with stage('read'):
                a, _ = sa.next(seg_bytes)
        finally:
            if ahead is not None:
                ahead.join()
        if a is None:
            return
        b = None
        if not b_ended:
            with stage('read'):
                b, _ = sb.next(len_bytes(a) + (1 << 16), a.n)
            if b is None or b.n < a.n:
                b_ended = True
        yield a, b


def _quietly(fn, *args):
    """fn(*args) on a helper thread: a failure is left for the main call on the same stream to meet and report."""
    try:
        fn(*args)
    except Exception:                        # noqa: BLE001
        pass


def len_bytes(reader):
    """Bytes of text a segment holds (what its follower is asked for first)."""
    return max(reader.record_offset(reader.first + reader.n) - reader.record_offset(reader.first), 1 << 16) if reader.n else 1 << 16


def _grown(tables, R, S2):
    """`tables` at (at least) R read groups and S2 cycle columns: the reference appends zeros at the END of either axis when
    a longer read or a new read group arrives (recalibrate.py:66-87), so every count keeps its absolute index."""
    if tables is not None and tables.R >= R and tables.S2 >= S2:
        return tables
    if tables is None:
        return dev.Tables(R, S2)
    R, S2 = max(R, tables.R), max(S2, tables.S2)
    old = tables.to_host()
    new = [np.zeros((R, 43, S2), dtype=np.int64), np.zeros((R, 43, S2), dtype=np.int64),
           np.zeros((R, 43, 16), dtype=np.int64), np.zeros((R, 43, 16), dtype=np.int64)]
    for o, w in zip(old, new):
        w[:o.shape[0], :, :o.shape[2]] = o
    return dev.Tables.from_host(*new)


class _Sequential:
    """The two passes over inputs that are READ SEQUENTIALLY (fastx.FastqStream): pipes, process substitutions, standard
    input -- and regular files when KBBQ_SEQUENTIAL is set: no mapping, no whole-file index, host memory a few segments
    whatever the input's size.  What the reference's walk carries from read to read (recalibrate.py:59-101: read groups in
    first-appearance order, the longest read so far, the growing count arrays) is carried from segment to segment; the
    first offending read stops the walk where the reference stops.  File A is needed twice: a regular file is read again,
    anything else is copied to a spool file while pass 1 reads it (KBBQ_SPOOL_DIR, default the temporary directory)."""

    def __init__(self, fastq, infer_rg):
        world, _ = parallel.world_rank()
        if world > 1:
            raise ValueError('inputs that are read sequentially (pipes, standard input) need a single process: the ranks of a '
                             'multi-GPU run cut their byte ranges out of regular files')
        self.fastq, self.infer_rg = fastq, infer_rg
        self.spool = None
        self.rgs, self.longest, self.total_a, self.usable = [], 0, 0, 0

    def rg_to_int(self):
        return {(nm if self.infer_rg else 0): i for i, nm in enumerate(self.rgs)}

    def close(self):
        if getattr(self, 'peak', None) is not None:
            self.peak.close()
            self.peak = None
        if self.spool is not None:
            try:
                os.unlink(self.spool)
            except OSError:
                pass
            self.spool = None

    def _open_a(self, spool=True):
        sa = fastx.FastqStream(self.fastq[0])
        fd = None
        if not sa.regular and spool:
            import tempfile
            fd, self.spool = tempfile.mkstemp(prefix='kbbq-spool-', suffix='.fq', dir=os.environ.get('KBBQ_SPOOL_DIR') or None)
            sa.tee(fd)
        return sa, fd

    def pass1(self, minscore=6, tally=True, spool=True):
        """Count tables of the pair (None when no read was tallied); tally=False: file A alone, read groups and the spool
        only (a model file replaces pass 1); spool=False: no pass 2 will follow (fastq_to_covariate_arrays)."""
        sa, fd = self._open_a(spool)
        sb = fastx.FastqStream(self.fastq[1]) if tally else None
        budget = dev.device_budget()
        self.peak = _stream.Peak(budget)
        tables, b_ended = None, False
        segments = _prefetched(_pair_segments(sa, sb, _segment_bytes()))
        try:
            for a, b in segments:
                self.total_a += a.n
                if tally and b is None:
                    b_ended = True                               # file B ended at the last segment's end
                if b_ended:
                    if sa.regular or not spool:
                        break                                    # zip() has stopped (H6) and file A can be read again (or is not needed again)
                    continue                                     # ... a pipe is drained into the spool for pass 2
                with stage('scan'):
                    usable, S_seg, R, kind, idx = a.scan_next(b, self.infer_rg, self.rgs, self.longest)
                self.rgs = a.rg_names()
                self.longest = max(self.longest, S_seg)
                if tally and usable > 0:
                    tables = _grown(tables, R, 2 * self.longest)
                    try:
                        _stream.tally_range(a, b, self.infer_rg, a.first, a.first + usable, tables, minscore, budget)
                    except (IndexError, TypeError) as e:
                        if hasattr(e, 'read_index'):
                            e.read_index = a.first + max(e.read_index, 0)
                        raise
                self.usable += usable
                if kind:
                    raise fastx._SCAN_ERRORS[kind](a.first + idx)
                if tally and (b is None or b.n < a.n):
                    b_ended = True
        finally:
            segments.close()                                     # joins the reading thread before the streams go
            if fd is not None:
                os.close(fd)
            sa.close()
            if sb is not None:
                sb.close()
        return tables

    def pass2(self, lut, shape, output, qmap=None):
        """Every read of file A (its own first-appearance read groups, recalibrate.py:141-148) through K2 and the writer.
        qmap: the device map of static quantized qualities (_stream.produce_range)."""
        from . import _egress
        torch = dev._torch()
        device = torch.cuda.current_device()
        budget = dev.device_budget()
        sa = fastx.FastqStream(self.spool or self.fastq[0])
        peak = self.peak = getattr(self, 'peak', None) or _stream.Peak(budget)
        infer_rg = self.infer_rg
        segments = _prefetched(_pair_segments(sa, None, _segment_bytes()))

        def produced():
            rgs = []
            for a, _ in segments:
                with stage('scan'):
                    _, _, _, kind, idx = a.scan_next(None, infer_rg, rgs, 0)
                if kind:
                    raise fastx._SCAN_ERRORS[kind](a.first + idx)
                rgs = a.rg_names()
                try:
                    yield from _stream.produce_range(a, infer_rg, a.first, a.first + a.n, lut, shape, budget, origin=a.first,
                                                     extra=dict(text=a, base=a.first), device=device, qmap=qmap)
                except _stream.REFUSALS as e:
                    if hasattr(e, 'read_index'):
                        e.read_index = a.first + max(e.read_index, 0)
                    raise
        try:
            widest = fastx.pitch_for(max(self.longest, 1)) * 2 + 16
            if output is None and _bgzf.enabled():
                with _bgzf.stdout_sink() as sink:
                    _egress.emit_produced(None, 0, produced(), widest, sink=sink)
            elif output is None:
                _egress.emit_produced(None, 0, produced(), widest)
            else:
                with _bgzf.open_sink(output) as sink:
                    _egress.emit_produced(None, 0, produced(), widest, sink=sink)
            LAST_RUN.clear()
            LAST_RUN['bands'] = []
            LAST_RUN['streamed'] = dict(peak.report(), reads=self.total_a, sequential=True, spooled=self.spool is not None,
                                        tables_bytes=8 * int(dev.N.load().kbbq_tables_count(shape[0], shape[2])), lut_bytes=int(lut.numel()))
        finally:
            try:
                segments.close()                                 # joins the reading thread before the stream goes
            except ValueError:                                   # (still running on the pipeline's thread: cannot happen once it has joined)
                pass
            sa.close()


def _recalibrate_sequential(fastq, infer_rg, gatkreport, output, quantize=None):
    """recalibrate_fastq for inputs that are read sequentially: same results, same errors at the same reads."""
    run = _Sequential(fastq, infer_rg)
    try:
        _warm_up()
        load = gatkreport is not None and os.path.exists(gatkreport)
        tables = run.pass1(tally=not load)
        if run.total_a == 0:
            return
        if load:
            tables = load_model(gatkreport, run.rg_to_int())
        elif tables is None:
            raise IndexError('index 0 is out of bounds for axis 0 with size 0')   # no read was tallied
        elif gatkreport is not None:
            save_model(tables, run.rg_to_int(), gatkreport)
        with stage('solve', sync=True):
            lut, shape = dev.solve_lut(tables)
        run.pass2(lut, shape, output, _device_qmap(quantize))
    finally:
        run.close()


def _emit_streamed(text, single, lut, shape, output, world, rank, qmap=None):
    """Pass 2 of a shard that is not resident (kbbq/_stream.py): file A's reads are filled again slab by slab and go through
    K2 while the slabs before them are copied back, rendered and written -- fill | H2D | K2 | D2H | format | write.  The
    ranks do not agree on a first error beforehand as the resident pass 2 does: an error stops the rank that meets it where
    it stands, after the records before the offending slab have been written (the reference prints up to the offending read)."""
    from . import _egress
    st = single['streamed']
    torch = dev._torch()
    device = torch.cuda.current_device()
    peak = st.get('peak') or _stream.Peak(st['budget'])
    try:
        produced = _stream.produce_range(st['A'], st['infer_rg'], st['lo'], st['hi'], lut, shape, st['budget'], device=device,
                                         qmap=qmap)
        widest = fastx.pitch_for(single['S']) * 2 + 16
        if output is None and _bgzf.enabled():
            def compressed():
                with _bgzf.stdout_sink() as sink:
                    _egress.emit_produced(text, single['first'], produced, widest, sink=sink)
            parallel.in_rank_order(compressed)
        elif output is None:
            parallel.in_rank_order(lambda: _egress.emit_produced(text, single['first'], produced, widest))
        else:
            with _bgzf.open_sink(output if world == 1 else '%s.rank%04d' % (output, rank)) as sink:
                _egress.emit_produced(text, single['first'], produced, widest, sink=sink)
        LAST_RUN.clear()
        LAST_RUN['bands'] = []
        LAST_RUN['streamed'] = dict(peak.report(), reads=st['hi'] - st['lo'],
                                    tables_bytes=8 * int(dev.N.load().kbbq_tables_count(shape[0], shape[2])), lut_bytes=int(lut.numel()))
    finally:
        peak.close()


BAM_TWO_COMMANDS = ('run the two commands instead: `kbbq bqsr -b aln.bam --kmers -g model.grp` on one GPU, then '
                    '`kbbq applybqsr -b aln.bam -g model.grp -o out.sam`, which runs under ranks')
_BAM_KMERS = 'recalibrate -b --kmers'


def _as_bam_kmers(exc):
    """A refusal of `bqsr --kmers` as the same exception naming this command."""
    text = str(exc.args[0]) if exc.args else ''
    return type(exc)(text.replace('bqsr --kmers', _BAM_KMERS) if 'bqsr --kmers' in text else '%s: %s' % (_BAM_KMERS, text))


def check_bam_kmers(bam, gatkreport=None, output=None, k=31, min_count=None, prefilter=False, filter_bits=4, partitions=1, passes=1,
                    exclude_flags=0, kmer_min_qual=None, kmers_from=None, bam_out=False, bam_index=None):
    """What recalibrate_bam refuses of its options, before the alignments are read, before any device work and, under a
    launcher, before the process group exists: a process group, what `bqsr --kmers` refuses of the k-mer options (the same
    exception types), an output name ending in .bam (without bam_out) and a report that exists.  kmers_from: k may then be None
    (the set's), and a counting option is refused (kmer.check_kmers_from).  bam_out: not with --bgzf.  bam_index: only with
    bam_out and an output name."""
    from . import kmer
    from .gatk import bqsr
    if parallel.launched_from_env() or kmer._ranks() is not None:
        raise ValueError('%s does not run across ranks yet (the k-mer table of the alignments is counted and read on one '
                         'GPU): on one GPU, or %s' % (_BAM_KMERS, BAM_TWO_COMMANDS))
    try:
        kmer.check_passes(passes)
        if kmer.check_kmers_from(kmers_from, prefilter, filter_bits, partitions, kmer_min_qual) is not None and k is None:
            k = 31                               # the set's: nothing to refuse here
        kmer._check_partitions(partitions)
        kmer.check_kmer_min_qual(kmer_min_qual)
        if not 8 <= int(k) <= 32:
            raise ValueError('k must be in 8..32, got %d' % int(k))
        if min_count is not None and int(min_count) < 1:
            raise ValueError('min_count must be >= 1, got %d' % int(min_count))
        if prefilter:
            kmer._check_prefilter(min_count, filter_bits)
        bqsr.check_exclude_flags(exclude_flags)
    except ValueError as exc:
        raise _as_bam_kmers(exc) from None
    if bam_out and _bgzf.enabled():
        raise ValueError('--bam-out: not with --bgzf (a BAM file is a BGZF file already)')
    if not bam_out and output is not None and str(output).lower().endswith('.bam'):
        raise ValueError('%s writes SAM text; BAM output (%s) is not supported' % (_BAM_KMERS, output))
    if bam_index is not None:
        applybqsr.check_bam_index_options(bam_index, bam_out, output)
    if gatkreport is not None and os.path.exists(gatkreport):
        raise ValueError('%s: the report %s exists: its model would replace the tally of the alignments\' own k-mers; give the '
                         'name of a report to write, or apply the report with `kbbq applybqsr`' % (_BAM_KMERS, gatkreport))


def check_bam_records(bam, use_oq=False, k=31, min_count=None, prefilter=False, filter_bits=4, mixed_lengths=False, exclude_flags=0):
    """What recalibrate_bam refuses of the records of an aln.AlignmentFile -- what `bqsr --kmers` refuses, with its exception
    types: several query lengths (without mixed_lengths), a record without RG, QUAL '*' without use_oq, a missing OQ tag with it
    (neither for a record that exclude_flags leaves out) -- on the reader's
    host arrays, before any device work.  Returns what gatk.bqsr._kmer_inputs returns: (batch, n, S), and the mask of the
    excluded records behind them with exclude_flags."""
    from .gatk import bqsr
    try:
        return bqsr._kmer_inputs(bam, k, min_count, prefilter, filter_bits, use_oq, 42, mixed_lengths, exclude_flags)
    except (ValueError, KeyError, TypeError) as exc:
        raise _as_bam_kmers(exc) from None


@_bgzf.option
def recalibrate_bam(bam, use_oq=False, set_oq=False, kmers=None, gatkreport=None, output=None, quantize=None, bam_out=False,
                    bam_index=None):
    """Without kmers: not implemented, as in the reference.
    bam: a path, or an aln.AlignmentFile.  kmers (a dict of bam_to_kmer_covariates' k-mer options: k, min_count, slots, prefilter, filter_bits, skip_unresolved, passes,
    partitions, mixed_lengths, exclude_flags, kmer_min_qual, kmers_from (a k-mer set file in the place of the count; k may then be None) -- a record that exclude_flags leaves out of the model is still recalibrated and
    written like any other): `kbbq bqsr -b bam --kmers ... [-u] -g R` and `kbbq applybqsr -b bam -g R [-u] [-s] [-o output]` in one run, the
    same bytes to stdout or `output` -- SAM text, the header as read.  The file is parsed once; SEQ and the source qualities
    (QUAL, or OQ with use_oq) go to the device once and the count, the flags, the tally (gatk.bqsr._kmer_tally) and the apply
    (kbbq_apply_aligned_dev, gatk.applybqsr._resident_slabs) read them there; the OQ plane follows for the context when records
    carry OQ tags and use_oq is not set.  The model is the one `applybqsr` would read from R: the tally's vectors as a report,
    its text parsed back (EstimatedQReported has four decimals there), get_delta_qs.  gatkreport: that text is written there;
    a report that exists is refused.  Refusals (check_bam_kmers, then check_bam_records) come before any
    device work.  quantize: the 256-byte map of gatk.applybqsr.quantize_map for the written QUAL (write_alignments); the tally,
    the report and the OQ tag of set_oq do not see it.  Returns `bqsr --kmers`'s info; LAST_RUN['aligned']: alignments, pitch, h2d_plane_bytes and planes, the planes
    that went to the device.  bam_out (--bam-out): the same records as a BAM file, whatever its name
    (gatk.applybqsr.write_alignments_bam): the resident SEQ plane and the apply's output plane are read where they lie; what BAM
    cannot hold is a ValueError before the tally and before the report or the file is created (kbbq._bamout.check).
    bam_index (--bam-index: auto, bai or csi; with bam_out and an output name): the file's index beside it, as
    gatk.applybqsr.apply_report makes it; alignments out of coordinate order are refused there too, before the tally."""
    if kmers is None:
        raise NotImplementedError('Recalibrating a bam is not yet implemented. '
                                  'Convert the BAM to FASTQ with `samtools fastq` first.')
    import sys
    from . import aln, kmer, recaltable
    from .gatk import bqsr
    quantize = applybqsr._check_qmap(quantize)
    opts = dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, skip_unresolved=False, passes=1, partitions=1,
                mixed_lengths=False, exclude_flags=0, kmer_min_qual=None, kmers_from=None)
    unknown = sorted(set(kmers) - set(opts))
    if unknown:
        raise TypeError('recalibrate_bam: unknown k-mer option %s' % ', '.join(unknown))
    opts.update(kmers)
    # (without the two options of the records every call below is the one it was)
    records = {key: opts[key] for key in ('mixed_lengths', 'exclude_flags') if opts[key]}
    check_bam_kmers(bam, gatkreport, output, opts['k'], opts['min_count'], opts['prefilter'], opts['filter_bits'],
                    opts['partitions'], opts['passes'], **{key: records[key] for key in ('exclude_flags',) if key in records},
                    **kmer._min_qual_kw(opts['kmer_min_qual']), **kmer._kmers_from_kw(opts['kmers_from']),
                    **({'bam_out': True} if bam_out else {}), **({} if bam_index is None else {'bam_index': bam_index}))
    given_k = opts['k']
    if opts['kmers_from'] is not None and given_k is None:
        opts['k'] = 31                           # for the refusals of the records; the tally takes the set's
    passes, partitions = kmer.check_passes(opts['passes']), kmer._check_partitions(opts['partitions'])
    if not isinstance(bam, aln.AlignmentFile):
        with stage('parse'):
            # (with bam_out and KBBQ_GPU_BAM=1: decoded on the device, the records kept for the writer -- kbbq/_bamin.py)
            bam = aln.alignments(bam, device=None if bam_out else False, keep_stream=True)
    inputs = check_bam_records(bam, use_oq, opts['k'], opts['min_count'], opts['prefilter'], opts['filter_bits'], **records)
    if bam_out:
        from . import _bamout
        _bamout.check(bam)
        if bam_index is not None:
            applybqsr.check_bam_index(bam, output, bam_index)
    info = {}
    with stage('k-mer tally', sync=True):
        vectors, resident = bqsr._kmer_tally(bam, inputs, given_k if given_k is None else int(given_k), opts['min_count'],
                                             opts['slots'], opts['prefilter'],
                                             opts['filter_bits'], use_oq, 6, 42, info, bool(opts['skip_unresolved']), passes, partitions,
                                             **kmer._min_qual_kw(opts['kmer_min_qual']), **kmer._kmers_from_kw(opts['kmers_from']))
    with stage('solve'):
        # the bytes of the report decide: what `applybqsr` reads back is the text, not the vectors
        text = str(bqsr.vectors_to_report(*vectors, list(utils.get_rg_to_pu(bam).values())))
        if gatkreport is not None:
            with open(gatkreport, 'w') as fh:
                fh.write(text)
        *model, rg_to_int = applybqsr._report_model(bam, recaltable.RecalibrationReport.fromtext(text))
    b, n, pitch = resident['batch'], resident['n'], resident['pitch']
    if not use_oq and bool((b.oq_len >= 0).any()):
        # records with an OQ tag take their context from it (gatk.applybqsr._rows): the one plane not there yet
        if hasattr(b, 'device_plane'):           # a DeviceBatch (kbbq/_bamin.py): the decode left it there
            resident['oq'] = b.device_plane(2, pitch)
        else:
            with stage('H2D', sync=True):
                resident['oq'] = dev._torch().from_numpy(b.plane(2, pitch)).cuda()
            resident['h2d_plane_bytes'] += n * pitch
        resident['planes'].append('OQ')
    kw = dict(use_oq=use_oq, set_oq=set_oq, resident=resident)
    if quantize is not None:                                 # without it the call is the one it was
        kw['quantize'] = quantize
    with stage('apply + render'):
        if bam_out:
            applybqsr.write_bam_file(bam, output, lambda writer: applybqsr.write_alignments_bam(bam, *model, rg_to_int, writer, **kw),
                                     **({} if bam_index is None else {'index': bam_index}))
        elif output is None and _bgzf.enabled():
            with _bgzf.stdout_sink() as sink:
                applybqsr.write_alignments(bam, *model, rg_to_int, sink, **kw)
        elif output is None:
            sys.stdout.flush()
            applybqsr.write_alignments(bam, *model, rg_to_int, sys.stdout.buffer, **kw)
            sys.stdout.flush()
        else:
            with _bgzf.open_sink(output) as sink:
                applybqsr.write_alignments(bam, *model, rg_to_int, sink, **kw)
    LAST_RUN.clear()
    LAST_RUN['aligned'] = dict(alignments=n, pitch=pitch, h2d_plane_bytes=resident['h2d_plane_bytes'], planes=list(resident['planes']))
    return info


@_bgzf.option
def recalibrate(bam, fastq, infer_rg=False, use_oq=False, set_oq=False, gatkreport=None, output=None, kmers=None, quantize=None):
    """Dispatcher of `kbbq recalibrate` (reference recalibrate.py:166-174).  The reference raises NotImplementedError
    for ANY gatkreport; here `-g` works with FASTQ input (a deliberate, documented divergence: SURVEY.md 8(f) #3), and
    the cases that stay unimplemented -- no FASTQ input, or a BAM without kmers -- raise NotImplementedError as the reference
    does.  kmers: recalibrate_bam's; with it a BAM is recalibrated from its own k-mers, and its info is returned.
    quantize: the 256-byte map of static quantized qualities (gatk.applybqsr.quantize_map) for whatever is written."""
    more = {} if quantize is None else dict(quantize=quantize)          # without it every call below is the one it was
    if kmers is not None and bam is not None:
        return recalibrate_bam(bam, use_oq, set_oq, kmers=kmers, gatkreport=gatkreport, output=output, **more)
    if kmers is not None:
        raise ValueError('kmers: only with a BAM (recalibrate -b --kmers); -c corrects and recalibrates a FASTQ file')
    if gatkreport is not None and fastq is None:
        raise NotImplementedError('GATKreport reading / creation is only implemented for FASTQ input (-f).')
    if bam is not None:
        recalibrate_bam(bam, use_oq, set_oq)
    elif fastq is not None:
        with stage('[recalibrate_fastq, wall]'):
            recalibrate_fastq(fastq, infer_rg=infer_rg, gatkreport=gatkreport, output=output, **more)
    else:
        raise ValueError('A BAM or FASTQ file should be provided for recalibration.')
