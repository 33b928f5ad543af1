"""Static quantized qualities on the MI355X (-m gpu): the plane kernel (kbbq_quantize_plane_dev) and the fused aligned apply
(kbbq_apply_aligned_q_dev / kbbq_apply_aligned_q) against the plain-Python map (tests/quantize_model.py), and every command that
takes --static-quantized-quals against the SAME command without it, the quality field of every record passed through that map."""
import ctypes
import sys

import numpy as np
import pytest

import quantize_model as Q
from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LEVELS = [10, 20, 30, 40]
WG_BYTES = 256 * 16                                  # one step of one workgroup: KQ_THREADS lanes x 16 bytes
WG_TILE = 8 * WG_BYTES                               # what the grid is sized by (KQ_CHUNKS_PER_LANE steps)


def _table(levels=LEVELS, round_down=False):
    return np.array(Q.model_map(levels, round_down), dtype=np.uint8)


# ---- the plane kernel ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def random_bytes():
    """Random bytes 0..255 for every plane size below, made once."""
    return np.random.default_rng(2024).integers(0, 256, size=400_000, dtype=np.uint8)


@pytest.mark.parametrize('nbytes', [16, WG_BYTES - 16, WG_BYTES, WG_BYTES + 16, WG_TILE - 16, WG_TILE + 16, 300 * 1024 + 48])
@pytest.mark.parametrize('which', ['levels', 'round-down', 'permutation'])
def test_plane_kernel(dev, random_bytes, nbytes, which):
    """In place, every byte through the table, nothing outside [0, nbytes) touched (16 guard bytes on either side).  The
    permutation is no quantization map: the kernel is a byte map and must serve any table."""
    import torch
    from kbbq import _native as N
    table = {'levels': _table(), 'round-down': _table(round_down=True),
             'permutation': np.random.default_rng(5).permutation(256).astype(np.uint8)}[which]
    assert nbytes % 16 == 0
    host = random_bytes[:nbytes + 32].copy()
    buf = torch.from_numpy(host).cuda()
    d_table = torch.from_numpy(table).cuda()
    ctx, lib = dev.context(), N.load()
    N.check(lib.kbbq_quantize_plane_dev(ctx.handle, ctypes.c_void_p(buf.data_ptr() + 16), nbytes, N.ptr(d_table)))
    ctx.status()
    got = buf.cpu().numpy()
    want = host.copy()
    want[16:16 + nbytes] = table[host[16:16 + nbytes]]
    assert np.array_equal(got[:16], host[:16]) and np.array_equal(got[16 + nbytes:], host[16 + nbytes:])
    assert np.array_equal(got, want)


def test_plane_kernel_arguments(dev):
    import torch
    from kbbq import _native as N
    ctx, lib = dev.context(), N.load()
    host = np.arange(64, dtype=np.uint8) + 40
    buf = torch.from_numpy(host.copy()).cuda()
    d_table = torch.from_numpy(_table()).cuda()
    assert lib.kbbq_quantize_plane_dev(ctx.handle, N.ptr(buf), 0, N.ptr(d_table)) == N.KBBQ_OK
    assert lib.kbbq_quantize_plane_dev(ctx.handle, None, 0, None) == N.KBBQ_OK
    assert lib.kbbq_quantize_plane_dev(ctx.handle, N.ptr(buf), 24, N.ptr(d_table)) == N.KBBQ_E_ARG
    assert lib.kbbq_quantize_plane_dev(ctx.handle, N.ptr(buf), -16, N.ptr(d_table)) == N.KBBQ_E_ARG
    assert lib.kbbq_quantize_plane_dev(ctx.handle, ctypes.c_void_p(buf.data_ptr() + 8), 16, N.ptr(d_table)) == N.KBBQ_E_ARG
    assert lib.kbbq_quantize_plane_dev(ctx.handle, N.ptr(buf), 16, None) == N.KBBQ_E_ARG
    with pytest.raises(ValueError, match='multiple of 16'):
        N.check(lib.kbbq_quantize_plane_dev(ctx.handle, N.ptr(buf), 24, N.ptr(d_table)))
    ctx.status()
    assert np.array_equal(buf.cpu().numpy(), host)                   # nothing was launched


def test_device_apply_takes_the_map(dev):
    """dev.apply / dev.apply_bands with qmap: the plane they return is the plane without it through the table -- plain rows,
    and the product's layout (mate-pair rows, 4-bit planes, grouped by read group) stored back in input order."""
    n, R, S = 2000, 2, 150
    batch = dev.ReadBatch.synthetic(0, n, n, seed=11, nrg=R)
    tables = dev.Tables(R, 2 * S)
    dev.accumulate(batch, tables)
    lut, shape = dev.solve_lut(tables)
    table = _table()
    qmap = dev.qmap_to_device(table)
    base = dev.apply(batch, lut, shape).cpu().numpy()
    got = dev.apply(batch, lut, shape, qmap=qmap).cpu().numpy()
    assert np.array_equal(got, table[base]) and not np.array_equal(got, base)
    laid = dev.lay_out(batch, R, S, packed=True)
    assert isinstance(laid, dev.PairBatch) and laid.seg is not None
    base2 = dev.apply(laid, lut, shape, restore_order=True).cpu().numpy()
    got2 = dev.apply(laid, lut, shape, restore_order=True, qmap=qmap).cpu().numpy()
    assert np.array_equal(got2, table[base2]) and not np.array_equal(got2, base2)
    base3 = dev.apply_bands([(laid, S, 0)], lut, shape, restore_order=True)[0].cpu().numpy()
    got3 = dev.apply_bands([(laid, S, 0)], lut, shape, restore_order=True, qmap=qmap)[0].cpu().numpy()
    assert np.array_equal(base3, base2) and np.array_equal(got3, got2)
    with pytest.raises(ValueError):
        dev.qmap_to_device(np.zeros(255, np.uint8))


# ---- the fused aligned apply -----------------------------------------------------------------------------------------------------

LENGTHS = [1, 15, 16, 17, 33, 150]


def _aligned_rows(seed, R=2, repeats=6):
    """Rows of every length in LENGTHS x forward / reverse x first / second of pair x R read groups, `repeats` of each, on
    character planes of pitch 160: the source qualities are QUAL, the context comes from a separate OQ plane."""
    rng = np.random.default_rng(seed)
    combos = [(L, flags, rg) for L in LENGTHS for flags in range(4) for rg in range(R)] * repeats
    order = rng.permutation(len(combos))
    L = np.array([combos[k][0] for k in order])
    flags = np.array([combos[k][1] for k in order])
    rg = np.array([combos[k][2] for k in order])
    n, pitch = len(combos), 160
    col = np.arange(pitch)[None, :] < L[:, None]
    seq = np.where(col, np.frombuffer(b'ACGTN', np.uint8)[rng.choice(5, (n, pitch), p=[.24, .24, .24, .24, .04])], 0).astype(np.uint8)
    qual = np.where(col, rng.integers(33 + 2, 33 + 42, (n, pitch)), 0).astype(np.uint8)
    oq = np.where(col, rng.integers(33 + 2, 33 + 42, (n, pitch)), 0).astype(np.uint8)
    meta = (L | (rg << 16) | (1 << 29) | ((flags & 1) << 30) | ((flags >> 1) << 31)).astype(np.uint32)
    return seq, qual, oq, meta


def _random_model(seed, R, S, kind):
    from test_gpu_applybqsr import _random_model as model
    return model(seed, R, S, kind)


class _Aligned:
    """The three device calls on one set of planes."""

    def __init__(self, dev, planes, model):
        import torch
        from kbbq import _native as N
        from kbbq.gatk import applybqsr
        self.N, self.torch = N, torch
        self.ctx, self.lib = dev.context(), N.load()
        self.host = planes
        seq, qual, oq, meta = planes
        self.n, self.pitch = seq.shape
        self.mode, blob, self.R, self.Qt, self.S2 = applybqsr._model(*model, 6)
        self.blob = blob
        self.d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (seq, qual, oq, meta.view(np.int32), blob)]

    def _args(self, d_out):
        N, d = self.N, self.d
        return (self.ctx.handle, N.ptr(d[0]), N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]), self.n, self.pitch, self.R, self.Qt, self.S2, 6,
                N.ptr(d[4]), self.mode, N.ptr(d_out))

    def run(self, table=None, q_call=True):
        """(output plane, status, row) of kbbq_apply_aligned_dev (q_call False) or kbbq_apply_aligned_q_dev with `table` (None: NULL)."""
        N = self.N
        d_out = self.torch.full_like(self.d[0], 0xEE)
        if not q_call:
            rc = self.lib.kbbq_apply_aligned_dev(*self._args(d_out))
        else:
            d_table = None if table is None else self.torch.from_numpy(table).cuda()
            rc = self.lib.kbbq_apply_aligned_q_dev(*self._args(d_out), N.ptr(d_table))
        N.check(rc)
        row = ctypes.c_int64(-1)
        status = self.lib.kbbq_ctx_status(self.ctx.handle, ctypes.byref(row))
        return d_out.cpu().numpy(), status, row.value


@pytest.mark.parametrize('kind,mode', [('int', 'KBBQ_ALIGNED_LUT'), ('float', 'KBBQ_ALIGNED_F64')])
def test_fused_aligned_apply(dev, kind, mode):
    from kbbq import _native as N
    planes = _aligned_rows(31)
    a = _Aligned(dev, planes, _random_model(13, 2, 150, kind))
    assert a.mode == {'KBBQ_ALIGNED_LUT': N.ALIGNED_LUT, 'KBBQ_ALIGNED_F64': N.ALIGNED_F64}[mode]
    base, status, _ = a.run(q_call=False)
    assert status == N.KBBQ_OK and not (base == 0xEE).any()
    L = planes[3] & 0xFFFF
    assert (base[np.arange(a.pitch)[None, :] >= L[:, None]] == 0).all()
    null, status, _ = a.run(None)
    assert status == N.KBBQ_OK and np.array_equal(null, base)         # a NULL map IS the existing call
    for round_down in (False, True):
        for levels in (LEVELS, [25], [7, 8, 9, 33, 34, 93]):
            table = _table(levels, round_down)
            got, status, _ = a.run(table)
            assert status == N.KBBQ_OK
            assert np.array_equal(got, table[base]), (levels, round_down)
            assert not np.array_equal(got, base)
    # preserved bases (source quality below 6) keep their byte, whatever the table says elsewhere
    kept = (planes[1] < 39) & (planes[1] > 0)
    assert kept.any() and np.array_equal(got[kept], planes[1][kept])


@pytest.mark.parametrize('kind', ['int', 'float'])
def test_fused_aligned_apply_decides_errors_before_the_map(dev, kind):
    """A new quality of about 250 (byte 283: KBBQ_E_RANGE) in one row, a source quality of 43 (>= Qt: KBBQ_E_INDEX) in another:
    the same status and the same row as the existing call, with a map that sends everything above 20 to 20 -- which would have
    'repaired' the out-of-range value had it been applied first."""
    from kbbq import _native as N
    seq, qual, oq, meta = _aligned_rows(37, R=3)
    model = _random_model(17, 3, 150, kind)
    model[0] = model[0].copy()
    model[0][2] = 250                                                 # read group 2: every new quality is out of range
    rg = (meta >> 16) & 0xFFF
    meta = np.where(rg == 2, meta & ~np.uint32(0xFFF << 16), meta).astype(np.uint32)      # nobody uses it ...
    table = _table([20])
    clean = _Aligned(dev, (seq, qual, oq, meta), model)
    base, status, _ = clean.run(q_call=False)
    assert status == N.KBBQ_OK
    got, status, _ = clean.run(table)
    assert status == N.KBBQ_OK and np.array_equal(got, table[base])
    long_rows = np.flatnonzero((meta & 0xFFFF) >= 33)
    r_range, r_index = int(long_rows[len(long_rows) // 2]), int(long_rows[len(long_rows) // 3])
    # ... but for one row
    m2 = meta.copy()
    m2[r_range] = (m2[r_range] & ~np.uint32(0xFFF << 16)) | np.uint32(2 << 16)
    q2 = qual.copy()
    q2[r_range, :20] = 33 + 30                                        # recalibrated bases, certainly
    a = _Aligned(dev, (seq, q2, oq, m2), model)
    want = a.run(q_call=False)
    assert want[1:] == (N.KBBQ_E_RANGE, r_range)
    got = a.run(table)
    assert got[1:] == want[1:]
    # a quality beyond the model's rows
    q3 = qual.copy()
    q3[r_index, 20] = 33 + 43
    a = _Aligned(dev, (seq, q3, oq, meta), model)
    want = a.run(q_call=False)
    assert want[1:] == (N.KBBQ_E_INDEX, r_index)
    got = a.run(table)
    assert got[1:] == want[1:]
    assert a.run(table)[1:] == want[1:]                               # the status words were reset in between
    assert clean.run(table)[1] == N.KBBQ_OK                           # nothing left behind


@pytest.mark.parametrize('kind', ['int', 'float'])
def test_host_buffer_form_equals_the_device_form(dev, monkeypatch, kind):
    """kbbq_apply_aligned_q with slabs of 1 MB (KBBQ_STAGE_MB; 8 000 rows x 160 bytes x 3 planes: several slabs), the table
    uploaded once with the model: the bytes of kbbq_apply_aligned_q_dev; with a NULL table those of kbbq_apply_aligned."""
    from kbbq import _native as N
    seq, qual, oq, meta = _aligned_rows(41, repeats=167)
    assert seq.shape[0] >= 8000
    a = _Aligned(dev, (seq, qual, oq, meta), _random_model(19, 2, 150, kind))
    table = _table(round_down=True)
    dev_form, status, _ = a.run(table)
    assert status == N.KBBQ_OK
    plain_dev, status, _ = a.run(q_call=False)
    assert status == N.KBBQ_OK

    def host_form(table, q_call=True):
        out = np.full_like(seq, 0xEE)
        bad = ctypes.c_int64(-2)
        args = (a.ctx.handle, N.ptr(seq), N.ptr(qual), N.ptr(oq), N.ptr(meta), a.n, a.pitch, a.R, a.Qt, a.S2, 6, N.ptr(a.blob),
                a.blob.nbytes, a.mode, N.ptr(out), ctypes.byref(bad))
        N.check(a.lib.kbbq_apply_aligned_q(*args, N.ptr(table)) if q_call else a.lib.kbbq_apply_aligned(*args))
        assert bad.value == -1
        return out
    monkeypatch.setenv('KBBQ_STAGE_MB', '1')
    for _ in range(2):                                                # a second call re-uses the staging
        assert np.array_equal(host_form(table), dev_form)
    assert np.array_equal(host_form(None), plain_dev)
    assert np.array_equal(host_form(None, q_call=False), plain_dev)
    monkeypatch.delenv('KBBQ_STAGE_MB')
    assert np.array_equal(host_form(table), dev_form)                 # one slab
    # a flagged row keeps its index in the whole input
    bad_q = qual.copy()
    bad_q[6001, 0] = 33 + 43
    monkeypatch.setenv('KBBQ_STAGE_MB', '1')
    bad = ctypes.c_int64(-2)
    out = np.empty_like(seq)
    rc = a.lib.kbbq_apply_aligned_q(a.ctx.handle, N.ptr(seq), N.ptr(bad_q), N.ptr(oq), N.ptr(meta), a.n, a.pitch, a.R, a.Qt, a.S2, 6,
                                    N.ptr(a.blob), a.blob.nbytes, a.mode, N.ptr(out), ctypes.byref(bad), N.ptr(table))
    assert rc == N.KBBQ_E_INDEX and bad.value == 6001
    a.ctx.status()


# ---- the commands ----------------------------------------------------------------------------------------------------------------

@pytest.fixture
def kbbq(monkeypatch, capfdbinary):
    """The command line in this process: main.main(argv), standard output and error dropped."""
    from kbbq import main
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                      # this process has torch tensors already
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED', 'KBBQ_DEVICE_BUDGET', 'KBBQ_SEQUENTIAL',
                'KBBQ_SEGMENT_BYTES'):
        monkeypatch.delenv(var, raising=False)

    def run(*argv):
        main.main([str(a) for a in argv])
        sys.stdout.flush()
        sys.stderr.flush()
        return capfdbinary.readouterr()
    return run


def _both(kbbq, tmp_path, argv, qopts, field, after=None):
    """The command without the option and with it, each to a file: (bytes without, bytes with); the bytes with the option must
    be those without it with every record's quality field through the model map.  after(): called after each run."""
    plain, quant = tmp_path / 'plain.out', tmp_path / 'quant.out'
    kbbq(*argv, '-o', plain)
    if after:
        after()
    kbbq(*argv, '-o', quant, *qopts)
    if after:
        after()
    levels, round_down = [], '--round-down-quantized' in qopts
    for k, x in enumerate(qopts):
        if x == '--static-quantized-quals':
            levels += [int(v) for v in qopts[k + 1].split(',')]
    a, b = plain.read_bytes(), quant.read_bytes()
    want = Q.map_quality_fields(a, Q.model_map(levels, round_down), field)
    assert len(a) > 0 and want != a, 'the fixture is degenerate: the map changes nothing'
    assert b == want
    return a, b


def _fastq(oracle, tmp_path, n, lo, hi, nrg, seed, names=None, sort=True):
    seq, cseq, qual, meta = oracle.synth(0, n, n, seed, lo, hi, nrg)
    if sort:
        order = np.argsort(meta & 0xFFFF, kind='stable')
        seq, cseq, qual, meta = seq[order], cseq[order], qual[order], meta[order]
    names = oracle.synth_names(0, n, nrg, with_rg=True) if names is None else names
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    return fa, fb


QOPTS = ('--static-quantized-quals', '10,20', '--static-quantized-quals', '30,40')
QDOWN = ('--static-quantized-quals', '12,25,37', '--round-down-quantized')


def test_recalibrate_f_one_band(dev, oracle, kbbq, tmp_path):
    from kbbq import recalibrate
    fa, fb = _fastq(oracle, tmp_path, 2000, 100, 100, 1, 3, names=['r%d' % i for i in range(2000)], sort=False)

    def one_band():
        assert len(recalibrate.LAST_RUN['bands']) == 1
    _both(kbbq, tmp_path, ['recalibrate', '-f', fa, fb], QDOWN, 'fastq', one_band)


def test_recalibrate_f_mixed_lengths_three_read_groups(dev, oracle, kbbq, tmp_path, monkeypatch):
    """Reads of 36..300 bases in non-decreasing order, 3 read groups: all length bands in one launch (dev.apply_bands), rows
    grouped by read group and stored back in input order."""
    from kbbq import recalibrate
    fa, fb = _fastq(oracle, tmp_path, 2400, 36, 300, 3, 5)
    seen = []
    real = dev.apply_bands

    def spy(items, *a, **kw):
        outs = real(items, *a, **kw)
        seen.append((len(items), kw.get('restore_order'), kw.get('qmap') is not None))
        return outs
    monkeypatch.setattr(dev, 'apply_bands', spy)
    _both(kbbq, tmp_path, ['recalibrate', '-f', fa, fb, '--infer-rg'], QOPTS, 'fastq')
    assert len(seen) == 2 and seen[0][0] >= 2 and seen[0][:2] == seen[1][:2] and seen[0][1] is True
    assert [s[2] for s in seen] == [False, True]
    assert len(recalibrate.LAST_RUN['bands']) >= 2


def test_recalibrate_f_mate_pair_rows(dev, oracle, kbbq, tmp_path):
    from kbbq import recalibrate
    fa, fb = _fastq(oracle, tmp_path, 2000, 100, 100, 2, 7)

    def pair_rows():
        bands = recalibrate.LAST_RUN['bands']
        assert len(bands) == 1 and 'mate-pair rows' in bands[0]['layout'] and bands[0]['output_rows'].startswith('mate-pair rows')
    _both(kbbq, tmp_path, ['recalibrate', '-f', fa, fb, '--infer-rg'], QOPTS, 'fastq', pair_rows)


def test_recalibrate_f_streamed_within_a_budget(dev, oracle, kbbq, tmp_path, monkeypatch):
    from kbbq import recalibrate
    fa, fb = _fastq(oracle, tmp_path, 2400, 60, 150, 3, 9)
    monkeypatch.setenv('KBBQ_DEVICE_BUDGET', '256K')

    def streamed():
        st = recalibrate.LAST_RUN['streamed']
        assert st['reads'] == 2400 and not st.get('sequential')
    _both(kbbq, tmp_path, ['recalibrate', '-f', fa, fb, '--infer-rg'], QOPTS, 'fastq', streamed)


def test_recalibrate_f_sequential(dev, oracle, kbbq, tmp_path, monkeypatch):
    from kbbq import recalibrate
    fa, fb = _fastq(oracle, tmp_path, 2400, 60, 150, 3, 11)
    monkeypatch.setenv('KBBQ_SEQUENTIAL', '1')
    monkeypatch.setenv('KBBQ_SEGMENT_BYTES', '64K')
    monkeypatch.setenv('KBBQ_DEVICE_BUDGET', '1M')

    def sequential():
        st = recalibrate.LAST_RUN['streamed']
        assert st['reads'] == 2400 and st['sequential']
    _both(kbbq, tmp_path, ['recalibrate', '-f', fa, fb, '--infer-rg'], QOPTS, 'fastq', sequential)


def test_recalibrate_c(dev, kbbq, tmp_path):
    import kmer_model as M
    from test_gpu_recalibrate_correct import _write
    seq, meta = M.synth(21, genome_len=6000, depth=30, err=0.01, len_lo=100, len_hi=100)[:2]
    n = seq.shape[0] & ~1
    fq = _write(tmp_path / 'pairs.fq', ['r%d/%d' % (i >> 1, (i & 1) + 1) for i in range(n)], seq[:n], meta[:n])
    _both(kbbq, tmp_path, ['recalibrate', '-c', fq], QOPTS, 'fastq')


@pytest.fixture(scope='module')
def alignments(tmp_path_factory):
    """2 000 alignments of one query length, 3 read groups, OQ tags (the k-mer tests' generator); every third record without its tag."""
    import oracle_bqsr as OQ
    from test_gpu_recalibrate_bam import _without_oq
    d = tmp_path_factory.mktemp('quantize_aln')
    sam = OQ.synth_bqsr_set(str(d), seed=11, npairs=1000, S=60, contigs=(('chr1', 2500), ('chr2', 2500)))['sam']
    text = open(sam).read()
    third = d / 'third.sam'
    third.write_text(_without_oq(text, lambda i: i % 3 != 0))
    return dict(all=sam, third=str(third))


def _oq_tags(text):
    return [[f for f in ln.split(b'\t')[11:] if f.startswith(b'OQ:Z:')] for ln in text.split(b'\n') if ln and not ln.startswith(b'@')]


@pytest.mark.parametrize('opts,qopts', [((), QOPTS), (('-s',), QOPTS), (('-u', '-s'), QDOWN)], ids=['plain', 's', 'u-s-round-down'])
def test_applybqsr(dev, kbbq, tmp_path, alignments, opts, qopts):
    """With -u every record carries its OQ tag here (a record without one passes through, and pass-through records are not
    quantized); without -u every third record lacks it and -s adds one holding the QUAL as read."""
    sam = alignments['all' if '-u' in opts else 'third']
    grp = tmp_path / 'model.grp'
    kbbq('bqsr', '-b', sam, '--kmers', '-k', '15', '-g', grp)
    a, b = _both(kbbq, tmp_path, ['applybqsr', '-b', sam, '-g', grp, *opts], qopts, 'sam')
    tags = _oq_tags(b)
    assert len(tags) == 2000 and tags == _oq_tags(a) and all(len(t) == 1 for t in tags) == ('-s' in opts or '-u' in opts)
    if '-s' in opts and '-u' not in opts:
        src = [ln.split(b'\t') for ln in open(sam, 'rb').read().split(b'\n') if ln and not ln.startswith(b'@')]
        added = [(t[0][5:], s[10]) for t, s in zip(tags, src) if not any(f.startswith(b'OQ:Z:') for f in s[11:])]
        assert len(added) >= 600 and all(x == y for x, y in added)    # the OQ tag holds the qualities as read, not the quantized ones


def test_applybqsr_passes_records_without_source_qualities_through(dev, kbbq, tmp_path, alignments):
    """-u on records without an OQ tag: nothing to recalibrate from, the QUAL as read goes out -- unquantized, as the rule says."""
    sam = alignments['third']
    grp = tmp_path / 'model.grp'
    kbbq('bqsr', '-b', alignments['all'], '--kmers', '-k', '15', '-u', '-g', grp)
    plain, quant = tmp_path / 'plain.sam', tmp_path / 'quant.sam'
    kbbq('applybqsr', '-b', sam, '-g', grp, '-u', '-o', plain)
    kbbq('applybqsr', '-b', sam, '-g', grp, '-u', '-o', quant, *QOPTS)
    table = Q.model_map(LEVELS)
    want, through = [], 0
    for ln in plain.read_bytes().split(b'\n'):
        if ln and not ln.startswith(b'@'):
            cols = ln.split(b'\t')
            if any(f.startswith(b'OQ:Z:') for f in cols[11:]):
                cols[10] = Q.map_bytes(cols[10], table)
            else:
                through += 1
            ln = b'\t'.join(cols)
        want.append(ln)
    assert through == len(range(0, 2000, 3)) and quant.read_bytes() == b'\n'.join(want) != plain.read_bytes()


def test_recalibrate_b_kmers(dev, kbbq, tmp_path, alignments):
    a, b = _both(kbbq, tmp_path, ['recalibrate', '-b', alignments['third'], '--kmers', '-k', '15', '-s'], QOPTS, 'sam')
    assert _oq_tags(a) == _oq_tags(b) and all(len(t) == 1 for t in _oq_tags(b))
    # the report is the one written without the option
    g1, g2 = tmp_path / 'one.grp', tmp_path / 'two.grp'
    kbbq('recalibrate', '-b', alignments['third'], '--kmers', '-k', '15', '-g', g1, '-o', tmp_path / 'x.sam')
    kbbq('recalibrate', '-b', alignments['third'], '--kmers', '-k', '15', '-g', g2, '-o', tmp_path / 'y.sam', *QOPTS)
    assert g1.read_bytes() == g2.read_bytes()
    assert (tmp_path / 'y.sam').read_bytes() == Q.map_quality_fields((tmp_path / 'x.sam').read_bytes(), Q.model_map(LEVELS), 'sam')
