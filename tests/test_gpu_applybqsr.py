"""
GPU tests (-m gpu) of ApplyBQSR on aligned reads: kbbq.gatk.applybqsr.recalibrate_alignments (kbbq_apply_aligned,
csrc/kbbq_apply_aligned.h) against the reference's goldens (tests/golden/bqsr_*: ab_recal) and against the per-read host
function recalibrate_bamread on random alignments; float models from a report, with and without the exact float64 path;
the reference's exceptions; the `kbbq bqsr` / `kbbq applybqsr` commands, on one process and on several ranks.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import dev                      # noqa: F401  (fixture)
from test_oracle_bqsr import VEC, _inputs

pytestmark = pytest.mark.gpu


def _per_read(reads, model, rg_to_int, use_oq):
    from kbbq.gatk import applybqsr
    return np.concatenate([applybqsr.recalibrate_bamread(r, model[0], *model[1:5], rg_to_int, use_oq=use_oq) for r in reads])


@pytest.mark.parametrize('name', ['bqsr_a', 'bqsr_b'])
def test_goldens(dev, oracle, name, tmp_path):
    import bamwriter
    from kbbq import aln, compare_reads
    from kbbq.gatk import applybqsr
    info, gold, paths = _inputs(name, tmp_path, oracle)
    vectors = [gold[k] for k in VEC]
    dqs = oracle.get_delta_qs(*vectors)
    for source in (paths['sam'], bamwriter.write_bam(tmp_path / 'a.bam', open(paths['sam']).read())):
        bam = aln.AlignmentFile(source)
        rg_to_int = {rg: i for i, rg in enumerate(compare_reads.get_rg_to_pu(bam))}
        got, off = applybqsr.recalibrate_alignments(bam, vectors[0], *dqs, rg_to_int)
        assert np.array_equal(got, gold['ab_recal'])
        assert off[-1] == got.size and len(off) == len(bam) + 1
        assert applybqsr.LAST_RUN['mode'] == 'lut'


def _random_sam(path, seed, n=400, S=40, nrg=3, longest=70, oq_missing=0.15, alphabet='ACGTN'):
    """Random alignments: both strands, first and second of pair, several read groups, lengths 1..longest, Ns, low qualities,
    OQ != QUAL, some records without OQ."""
    rng = np.random.default_rng(seed)
    lines = ['@HD\tVN:1.6', '@SQ\tSN:c\tLN:100000'] + ['@RG\tID:g%d\tPU:u%d' % (g, g) for g in range(nrg)]
    for i in range(n):
        L = int(rng.integers(1, longest + 1))
        flag = int(rng.choice([0, 16])) | int(rng.choice([64, 128])) | 1
        seq = ''.join(rng.choice(list(alphabet), size=L, p=None))
        qual = ''.join(chr(33 + int(q)) for q in rng.integers(2, 43, size=L))
        oq = ''.join(chr(33 + int(q)) for q in rng.integers(0, 43, size=L))
        tags = ['RG:Z:g%d' % rng.integers(nrg)]
        if rng.random() >= oq_missing:
            tags.insert(int(rng.integers(2)), 'OQ:Z:' + oq)
        lines.append('\t'.join(['r%d' % i, str(flag), 'c', str(1 + i), '60', '%dM' % L, '*', '0', '0', seq, qual] + tags))
    path.write_text('\n'.join(lines) + '\n')
    return str(path)


def _random_model(seed, R, S, kind='int'):
    rng = np.random.default_rng(seed)
    meanq = rng.integers(20, 35, size=R) if kind == 'int' else rng.uniform(20, 35, size=R)
    rgdq = rng.integers(-2, 3, size=R)
    qdq = rng.integers(-4, 5, size=(R, 43))
    posdq = rng.integers(-3, 4, size=(R, 43, 2 * S))
    dndq = np.concatenate([rng.integers(-3, 4, size=(R, 43, 16)), np.zeros((R, 43, 1), np.int64)], axis=-1)
    if kind == 'float':
        rgdq, qdq, posdq, dndq = (x + rng.uniform(-0.5, 0.5, size=x.shape) for x in (rgdq, qdq, posdq, dndq))
        dndq[..., 16] = 0.0
    return [meanq, rgdq, qdq, posdq, dndq]


def _host_reference(bam, model, rg_to_int, use_oq):
    """recalibrate_bamread read by read; a read without OQ is compared as a copy whose OQ is its source qualities (use_oq=False)
    or passes through unchanged (use_oq=True)."""
    from kbbq.gatk import applybqsr
    out = []
    for r in bam:
        if not r.has_tag('OQ'):
            if use_oq:
                out.append(np.array(r.query_qualities, dtype=np.int_))
                continue
            r.set_tag('OQ', ''.join(chr(33 + q) for q in r.query_qualities))
        out.append(applybqsr.recalibrate_bamread(r, model[0], *model[1:5], rg_to_int, use_oq=use_oq))
    return np.concatenate(out)


@pytest.mark.parametrize('use_oq', [True, False])
@pytest.mark.parametrize('kind', ['int', 'float'])
def test_against_the_per_read_function(dev, tmp_path, use_oq, kind):
    import bamwriter
    from kbbq import aln
    from kbbq.gatk import applybqsr
    sam = _random_sam(tmp_path / 'r.sam', seed=5 + use_oq)
    model = _random_model(7, 3, 40, kind)
    rg_to_int = {'g0': 0, 'g1': 1, 'g2': 2}
    for source in (sam, bamwriter.write_bam(tmp_path / 'r.bam', open(sam).read())):
        bam = aln.AlignmentFile(source)
        got, off = applybqsr.recalibrate_alignments(bam, *model, rg_to_int, use_oq=use_oq)
        want = _host_reference(aln.AlignmentFile(source), model, rg_to_int, use_oq)
        assert np.array_equal(got, want)
        assert np.array_equal(np.diff(off), [len(r.query_sequence) for r in bam])


def test_float_model_from_a_report(dev, oracle, tmp_path):
    """bam_to_report -> report file -> table_to_vectors -> get_delta_qs (float64 deltas) -> the kernel, per read against the host
    sum; then a hand-made model whose levels sit a few ulps off an integer and whose totals go negative: the exact float64
    path runs, and still equals the host."""
    from kbbq import aln, benchmark
    from kbbq.gatk import applybqsr, bqsr
    info, gold, paths = _inputs('bqsr_a', tmp_path, oracle)
    rep = tmp_path / 'a.grp'
    bqsr.bam_to_report(aln.AlignmentFile(paths['sam']), paths['fa'], benchmark.get_var_sites(paths['vcf'])).write(str(rep))
    bam = aln.AlignmentFile(paths['sam'])
    *model, rg_to_int = applybqsr.report_model(bam, str(rep))
    assert model[0].dtype == np.float64
    got, _ = applybqsr.recalibrate_alignments(bam, *model, rg_to_int, use_oq=True)
    assert np.array_equal(got, _per_read(list(bam), model, rg_to_int, True))

    # adversarial: base = meanq + rgdq + qdq lands a few ulps below / above integers; a negative level
    R = len(rg_to_int)
    S = model[3].shape[2] // 2
    meanq = np.array([30.0 - 2 ** -40, 12.0 + 2 ** -45, 40.0 + 1e-13][:R])
    rgdq = np.zeros(R)
    qdq = np.zeros((R, 43))
    qdq[:, 30:] = -40.0                           # totals below zero (no clipping: trunc toward zero)
    posdq = np.tile(np.linspace(-1.0, 1.0, 2 * S), (R, 43, 1))
    dndq = np.zeros((R, 43, 17))
    dndq[..., :16] = np.linspace(0, 2, 16) + 2 ** -44
    adv = [meanq, rgdq, qdq, posdq, dndq]
    got, _ = applybqsr.recalibrate_alignments(bam, *adv, rg_to_int, use_oq=True)
    assert applybqsr.LAST_RUN['mode'] == 'f64'
    want = _per_read(list(bam), adv, rg_to_int, True)
    assert (want < 0).any() and np.array_equal(got, want)


def _one_read_sam(path, seq, qual, flag=0, rg='g0', extra=()):
    lines = ['@HD\tVN:1.6', '@RG\tID:g0\tPU:u0', '@RG\tID:g1\tPU:u1']
    good = 'ok\t0\tc\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tOQ:Z:IIII\tRG:Z:g0'
    tags = ['OQ:Z:' + qual] + (['RG:Z:' + rg] if rg else [])
    lines += [good, good, '\t'.join(['bad', str(flag), 'c', '1', '60', '%dM' % len(seq), '*', '0', '0', seq, qual] + tags), good]
    path.write_text('\n'.join(lines + list(extra)) + '\n')
    return str(path)


@pytest.mark.parametrize('case, exc', [
    (dict(seq='ACGT', qual='II' + chr(33 + 43) + 'I'), IndexError),           # q >= 43
    (dict(seq='A' * 9, qual='I' * 9), IndexError),                            # longer than 2S (S = 4)
    (dict(seq='ACGT', qual='IIII', rg='nope'), KeyError),                      # unknown read group
    (dict(seq='ACGT', qual='IIII', rg=None), KeyError),                        # no RG tag
    (dict(seq='ACRT', qual='IIII'), TypeError),                                # IUPAC letter, forward strand
])
def test_errors(dev, tmp_path, case, exc):
    from kbbq import aln
    from kbbq.gatk import applybqsr
    sam = _one_read_sam(tmp_path / 'e.sam', **case)
    model = _random_model(3, 2, 4)
    rg_to_int = {'g0': 0, 'g1': 1}
    reads = list(aln.AlignmentFile(sam))
    with pytest.raises(exc):
        applybqsr.recalibrate_bamread(reads[2], model[0], *model[1:], rg_to_int)
    with pytest.raises(exc) as e:
        applybqsr.recalibrate_alignments(aln.AlignmentFile(sam), *model, rg_to_int)
    assert e.value.read_index == 2


def test_iupac_on_the_reverse_strand_is_an_n(dev, tmp_path):
    from kbbq import aln
    from kbbq.gatk import applybqsr
    sam = _one_read_sam(tmp_path / 'e.sam', seq='ACRTGGAYC', qual='IIIIIIIII', flag=16)
    model = _random_model(3, 2, 8)
    rg_to_int = {'g0': 0, 'g1': 1}
    got, _ = applybqsr.recalibrate_alignments(aln.AlignmentFile(sam), *model, rg_to_int)
    assert np.array_equal(got, _per_read(list(aln.AlignmentFile(sam)), model, rg_to_int, True))


def _kbbq(*argv, timeout=300):
    import subprocess
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=env)


def _quals_of(line):
    return np.frombuffer(line.split('\t')[10].encode(), dtype=np.uint8).astype(np.int_) - 33


def test_command_line(dev, oracle, tmp_path):
    from kbbq import aln
    from kbbq.gatk import applybqsr
    from test_gpu_ranks import _run_ranks
    info, gold, paths = _inputs('bqsr_a', tmp_path, oracle)
    rep = str(tmp_path / 'a.grp')
    r = _kbbq('bqsr', '-b', paths['sam'], '-r', paths['fa'], '-v', paths['vcf'], '-g', rep)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text = open(rep).read()
    assert len(text) == info['report_len'] and oracle.sha256(text) == info['report_sha256']

    # a copy of the input in which every third record lacks its OQ tag (-s adds one)
    src = open(paths['sam']).read().splitlines()
    edited = [('\t'.join(x for x in ln.split('\t') if not x.startswith('OQ:Z:')) if not ln.startswith('@') and k % 3 == 0 else ln)
              for k, ln in enumerate(src)]
    sam = tmp_path / 'in.sam'
    sam.write_text('\n'.join(edited) + '\n')
    bam = aln.AlignmentFile(str(sam))
    *model, rg_to_int = applybqsr.report_model(bam, rep)
    for opts in ([], ['-s'], ['-u', '-s']):
        out = tmp_path / ('o%d.sam' % len(opts))
        r = _kbbq('applybqsr', '-b', str(sam), '-g', rep, '-o', str(out), *opts)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = open(out).read().splitlines()
        assert len(got) == len(edited)
        reads = list(aln.AlignmentFile(str(sam)))
        k = 0
        for a, b in zip(edited, got):
            if a.startswith('@'):
                assert a == b
                continue
            read = reads[k]; k += 1
            fa, fb = a.split('\t'), b.split('\t')
            had_oq = read.has_tag('OQ')
            assert fa[:10] == fb[:10] and fa[11:] == fb[11:len(fa)]
            if '-s' in opts and not had_oq:
                assert fb[len(fa):] == ['OQ:Z:' + fa[10]]
            else:
                assert len(fb) == len(fa)
            if '-u' in opts and not had_oq:
                assert fb[10] == fa[10]                       # nothing to recalibrate from: passed through
                continue
            if not had_oq:
                read.set_tag('OQ', fa[10])
            want = applybqsr.recalibrate_bamread(read, model[0], *model[1:5], rg_to_int, use_oq='-u' in opts)
            assert np.array_equal(_quals_of(b), want)
    # stdout, the same bytes
    r = _kbbq('applybqsr', '-b', str(sam), '-g', rep)
    assert r.returncode == 0 and r.stdout == open(tmp_path / 'o0.sam', 'rb').read()
    # BAM output is refused
    r = _kbbq('applybqsr', '-b', str(sam), '-g', rep, '-o', str(tmp_path / 'x.bam'))
    assert r.returncode != 0 and b'BAM output' in r.stderr and not (tmp_path / 'x.bam').exists()
    # three ranks sharing the GPU: the rank files, concatenated in rank order, are the single-process output
    out = str(tmp_path / 'ranks.sam')
    r = _run_ranks(3, ['applybqsr', '-b', str(sam), '-g', rep, '-o', out, '-s'])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    joined = b''.join(open('%s.rank%04d' % (out, k), 'rb').read() for k in range(3))
    assert joined == open(tmp_path / 'o1.sam', 'rb').read()


def _synthetic_alignments(n, L, R, seed, separate_oq):
    """n alignments of L bases on host character planes (as scripts/time_applybqsr.py builds them on the device): both strands,
    first and second of pair, R read groups; the source qualities are QUAL with the context from a separate OQ plane, or one
    plane that is both."""
    rng = np.random.default_rng(seed)
    pitch = (L + 15) // 16 * 16
    col = np.arange(pitch)[None, :] < L
    seq = np.where(col, np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, (n, pitch))], 0).astype(np.uint8)
    qual = np.where(col, rng.integers(33 + 2, 33 + 42, (n, pitch)), 0).astype(np.uint8)
    oq = np.where(col, rng.integers(33 + 2, 33 + 42, (n, pitch)), 0).astype(np.uint8) if separate_oq else qual
    flags, rg = rng.integers(0, 4, n), rng.integers(0, R, n)
    meta = (L | (rg << 16) | (0 if separate_oq else 1 << 28) | (1 << 29) | ((flags & 1) << 30) | ((flags >> 1) << 31)).astype(np.uint32)
    return seq, qual, oq, meta


@pytest.mark.parametrize('separate_oq', [False, True])
@pytest.mark.parametrize('kind', ['int', 'float'])
def test_host_buffer_aligned_entry_runs_slab_by_slab(dev, monkeypatch, separate_oq, kind):
    """kbbq_apply_aligned moves a caller's rows through the page-locked slabs of kbbq_apply: with slabs of about two thousand
    rows -- KBBQ_STAGE_MB -- the bytes are those of a single-slab run and of kbbq_apply_aligned_dev on the same rows, and a row the
    kernel flags is reported with its index in the WHOLE input, in the message and in *bad_read."""
    import ctypes
    import re
    import torch
    from kbbq import _native as N
    from kbbq.gatk import applybqsr
    n, L, R = 30_001, 150, 3
    seq, qual, oq, meta = _synthetic_alignments(n, L, R, 11 + separate_oq, separate_oq)
    pitch = seq.shape[1]
    mode, blob, R_, Qt, S2 = applybqsr._model(*_random_model(13, R, L, kind), 6)
    assert mode == (N.ALIGNED_LUT if kind == 'int' else N.ALIGNED_F64)
    ctx, lib = dev.context(), N.load()

    def run(q, o, bad=None):
        out = np.full_like(seq, 0xEE)
        bad_read = ctypes.c_int64(-2)
        rc = lib.kbbq_apply_aligned(ctx.handle, N.ptr(seq), N.ptr(q), N.ptr(o), N.ptr(meta), n, pitch, R_, Qt, S2, 6,
                                    N.ptr(blob), blob.nbytes, mode, N.ptr(out), ctypes.byref(bad_read))
        if bad is None:
            N.check(rc)
            assert bad_read.value == -1
            return out
        with pytest.raises(IndexError) as e:
            N.check(rc)
        assert int(re.search(r'read (\d+)', str(e.value)).group(1)) == bad and bad_read.value == bad
        return None

    monkeypatch.delenv('KBBQ_STAGE_MB', raising=False)                # one slab (the default 96 MB)
    whole = run(qual, oq)
    monkeypatch.setenv('KBBQ_STAGE_MB', '1')                          # 1 MB per slab: ~2 100 rows of 160 bytes x 3 planes
    for _ in range(2):                                                # a second call re-uses the staging
        assert np.array_equal(run(qual, oq), whole)
    assert not (whole == 0xEE).any() and (whole[:, L:] == 0).all()
    d = [torch.from_numpy(x).cuda() for x in (seq, qual, oq, meta.view(np.int32), blob)]
    d_out = torch.full_like(d[0], 0xEE)
    N.check(lib.kbbq_apply_aligned_dev(ctx.handle, N.ptr(d[0]), N.ptr(d[1]), N.ptr(d[2] if separate_oq else d[1]), N.ptr(d[3]), n,
                                       pitch, R_, Qt, S2, 6, N.ptr(d[4]), mode, N.ptr(d_out)))
    ctx.status()
    assert np.array_equal(d_out.cpu().numpy(), whole)
    # a quality above 42 (IndexError of the reference) in a late slab, an earlier slab clean; then a second one before it
    bad = qual.copy()
    for first in (25_000, 7_777):
        bad[first, 3] = 33 + 43                                       # the source plane (with one plane: source and context)
        run(bad, oq if separate_oq else bad, first)
    ctx.status()                                                      # nothing left behind
