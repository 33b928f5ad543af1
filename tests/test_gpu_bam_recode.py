"""BAM recode on the GPU: the recode kernels (kbr_size, the scan, kbr_write) against their host twin byte for byte on the cases and
ranges of tests/bam_recode_cases.py with poisoned and guarded outputs; recode -> assemble against the host route's stream; and the
commands -- `applybqsr --bam-out`, `recalibrate -b --kmers --bam-out` -- in child processes with KBBQ_GPU_BAM=1 and without it:
the same file bytes, index bytes and stderr, route `device` with the variable and `host` without, and every case that stays with
the reader."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_in_cases as I
import bam_index_cases as K
import bam_out_cases as O
import bam_recode_cases as C
import bamwriter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED', 'KBBQ_GPU_BAM', 'KBBQ_STAGE_MB', 'KBBQ_DEVICE_BUDGET'):
    ENV.pop(_var, None)


def _raw(img):
    return np.frombuffer(img, dtype=np.uint8)


def _scan(img):
    from kbbq import _bamin as B
    return B.Scan(_raw(img))


def _up(a):
    from kbbq import _device as dev
    return dev._torch().from_numpy(np.array(a)).cuda()


def recode_device(img, scan, first, m, set_oq, keep, cap=None):
    """kbbq_bam_recode_dev on records [first, first + m), every output poisoned between guards: bam_recode_cases.result()."""
    from kbbq import _device as dev
    from kbbq import _native as N
    cap = C.skel_cap(scan, first, m, set_oq) if cap is None else cap
    (desc, at), (status, _), (skel, _) = C.guarded(24 * m), C.guarded(4 * m), C.guarded(cap)
    d_img, d_rec = _up(_raw(img)), _up(np.ascontiguousarray(scan.rec_off, dtype=np.uint64).view(np.int64))
    d_desc, d_status, d_skel = _up(desc), _up(status), _up(skel)
    d_keep = None if keep is None else _up(np.ascontiguousarray(keep, dtype=np.uint8))
    sb, tb, any_status = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0)
    rc = N.load().kbbq_bam_recode_dev(dev.context().handle, N.ptr(d_img), len(img), N.ptr(d_rec), first, m, int(set_oq), N.ptr(d_keep),
                                      scan.n_ref, N.ptr(d_desc.data_ptr() + at), N.ptr(d_skel.data_ptr() + at), cap,
                                      N.ptr(d_status.data_ptr() + at), ctypes.byref(sb), ctypes.byref(tb), ctypes.byref(any_status))
    return C.result(d_desc.cpu().numpy(), d_status.cpu().numpy(), d_skel.cpu().numpy(), m, cap, sb.value, tb.value, any_status.value, rc)


def _same(got, want, what):
    for key in ('rc', 'any', 'skel_bytes', 'stream_bytes'):
        assert got[key] == want[key], (key, what)
    for key in ('desc', 'status', 'skel'):
        assert np.array_equal(got[key], want[key]), (key, what)


@pytest.mark.parametrize('name', C.ALL)
def test_kernel_equals_host_twin(name):
    img, _ = C.named(name)
    scan = _scan(img)
    for set_oq in (0, 1):
        for kind, keep in C.keep_patterns(scan.n).items():
            _same(recode_device(img, scan, 0, scan.n, set_oq, keep), C.recode_host(img, scan, 0, scan.n, set_oq, keep), (name, set_oq, kind))


@pytest.mark.parametrize('m', C.COUNTS)
def test_kernel_equals_host_twin_on_record_ranges(m):
    img, _ = C.named('many')
    scan = _scan(img)
    for first in (0, 311):
        for set_oq in (0, 1):
            keep = C.keep_patterns(m)['alternating']
            _same(recode_device(img, scan, first, m, set_oq, keep), C.recode_host(img, scan, first, m, set_oq, keep), (first, m, set_oq))


def test_the_scan_over_many_workgroups():
    """3,000 records: twelve workgroups of the scan; and the sizes-only call."""
    img = I.image('trims')
    scan = _scan(img)
    want = C.recode_host(img, scan, 0, scan.n, 1, None)
    _same(recode_device(img, scan, 0, scan.n, 1, None), want, 'trims')
    sizes = recode_device(img, scan, 0, scan.n, 1, None, cap=0)
    assert sizes['rc'] == -4 and np.array_equal(sizes['desc'], want['desc']) and len(sizes['skel']) == 0


@pytest.mark.parametrize('kind', I.CORRUPTIONS)
def test_kernel_equals_host_twin_on_damaged_records(kind):
    img, row, bit = I.corrupted(kind)
    scan = _scan(img)
    for set_oq in (0, 1):
        got = recode_device(img, scan, 0, scan.n, set_oq, np.array([0, 1, 1], np.uint8))
        assert got['any'] == bit and got['status'][row] == bit
        _same(got, C.recode_host(img, scan, 0, scan.n, set_oq, np.array([0, 1, 1], np.uint8)), (kind, set_oq))


@pytest.mark.parametrize('name', ['many', 'quals', 'shapes', 'int_places', 'other_tags', 'in_lengths', 'in_count257'])
def test_recode_then_assemble_is_the_host_routes_stream(name, tmp_path):
    from kbbq import _device as dev
    from kbbq import _native as N
    img, _ = C.named(name)
    scan = _scan(img)
    bam = C.reader(tmp_path, img, 'x')
    rng = np.random.default_rng(5)
    seq, out, keep, pitch = O.planes(bam, rng)
    d_seq, d_out = _up(seq), _up(out)
    for set_oq in (0, 1):
        want, bad = O.host_stream(bam, seq, out, pitch, set_oq, keep)
        assert bad == -1
        got = recode_device(img, scan, 0, scan.n, set_oq, keep)
        assert got['any'] == 0 and got['stream_bytes'] == len(want)
        d_desc, d_skel = _up(got['desc'].reshape(-1).view(np.uint8)), _up(np.concatenate([got['skel'], np.zeros(16, np.uint8)]))
        d_stream = _up(np.full(len(want) + 64, C.POISON, np.uint8))
        row = ctypes.c_int64(-1)
        N.check(N.load().kbbq_bam_assemble_dev(dev.context().handle, N.ptr(d_skel), got['skel_bytes'], N.ptr(d_desc), scan.n, N.ptr(d_seq),
                                               N.ptr(d_out), pitch, N.ptr(d_stream), 0, len(want), ctypes.byref(row)))
        stream = d_stream.cpu().numpy()
        assert row.value == -1 and stream[:len(want)].tobytes() == want and (stream[len(want):] == C.POISON).all(), (name, set_oq)


# ---- the commands -------------------------------------------------------------------------------------------------------------------
# a child of its own, as the command line starts: the command, then the route and what went up for the BAM on stdout
CHILD = ('import sys\nfrom kbbq import aln, main\nfrom kbbq.gatk import applybqsr\n'
         'try:\n    main.main(sys.argv[1:])\nfinally:\n    sys.stdout.flush()\n    sys.stderr.flush()\n'
         '    run = aln.LAST_RUN.get("bam_in", {})\n'
         '    print("route=%s|fallback=%s|h2d=%s" % (run.get("route"), run.get("fallback"), applybqsr.LAST_RUN.get("bam_out", {}).get("h2d_bytes")))\n')


def _kbbq(*argv, device=False, env=None, ok=True):
    env = dict(ENV, **(env or {}), **({'KBBQ_GPU_BAM': '1'} if device else {}))
    r = subprocess.run([sys.executable, '-c', CHILD] + [str(a) for a in argv], capture_output=True, timeout=300, env=env)
    assert (r.returncode == 0) == ok, r.stderr.decode()[-3000:]
    said = dict(x.split('=', 1) for x in r.stdout.decode().strip().split('\n')[-1].split('|'))
    return said, r.stderr.decode()


def _report(path, rng, S2):
    from kbbq.gatk import bqsr
    R, Q = 3, 43
    q_total = rng.integers(0, 5000, (R, Q))
    q_errs = (q_total * rng.uniform(0, 0.05, (R, Q))).astype(np.int64)
    pos_total = rng.integers(0, 200, (R, Q, S2))
    pos_errs = (pos_total * rng.uniform(0, 0.1, (R, Q, S2))).astype(np.int64)
    dn_total = rng.integers(0, 800, (R, Q, 16))
    dn_errs = (dn_total * rng.uniform(0, 0.1, (R, Q, 16))).astype(np.int64)
    report = bqsr.vectors_to_report(np.zeros(R), q_errs.sum(1), q_total.sum(1), q_errs, q_total, pos_errs, pos_total, dn_errs, dn_total,
                                    ['pu0', 'pu1', 'pu2'])
    path.write_text(str(report))
    return str(path)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """3,000 random records (lengths 1..70, some without OQ, some with QUAL '*') and 2,000 sorted ones (90..150 bases), as BAM and
    as SAM; a report for each; the k-mer set of tests/test_gpu_bam_in.py."""
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('bam_recode')
    rng = np.random.default_rng(21)
    text = O.sam_text(O.random_records(rng, 3000))
    (d / 'random.sam').write_text(text)
    sorted_text = O.sam_text(K.many(rng, 2000), K.HEADER)
    kmers = OQ.synth_bqsr_set(str(d), seed=11, npairs=1500, S=60, contigs=(('chr1', 4000), ('chr2', 3500)))
    return dict(dir=d, sam=str(d / 'random.sam'), bam=str(bamwriter.write_bam(d / 'random.bam', text)), text=text,
                sorted=str(bamwriter.write_bam(d / 'sorted.bam', sorted_text)), kmers=str(bamwriter.write_bam(d / 'kmers.bam', open(kmers['sam']).read())),
                report=_report(d / 'random.grp', rng, 140), sorted_report=_report(d / 'sorted.grp', rng, 300))


def _both(files, tmp_path, argv, outputs=('out.bam',), source='bam'):
    """The command on both routes: {device: (the output files' bytes, stderr)}; asserts the routes."""
    got = {}
    for device in (False, True):
        d = tmp_path / ('device' if device else 'host')
        d.mkdir()
        said, err = _kbbq(*[str(a).replace('OUT', str(d)).replace('IN', files[source]) for a in argv], device=device)
        assert said['route'] == ('device' if device else 'host'), said
        got[device] = ([(d / name).read_bytes() for name in outputs], err, said)
    assert got[True][:2] == got[False][:2]
    return got


@pytest.mark.parametrize('opts', [(), ('-u',), ('-s',), ('-u', '-s'), ('--static-quantized-quals', '10,20,30')],
                         ids=['plain', 'u', 's', 'u-s', 'quantized'])
def test_applybqsr_both_ways(files, tmp_path, opts):
    got = _both(files, tmp_path, ['applybqsr', '-b', 'IN', '-g', files['report'], *opts, '--bam-out', '-o', 'OUT/out.bam'])
    data = got[True][0][0]
    assert len(data) > 100000 and data.endswith(bamwriter.bgzf(b'')[-28:])
    # no skeleton went up: the header and a keep byte per record, where the host route sends descriptors and skeleton too
    up_device, up_host = int(got[True][2]['h2d']), int(got[False][2]['h2d'])
    assert up_device < 3000 + 2000 and up_host > 3000 * 24 + up_device


@pytest.mark.parametrize('kind', ['bai', 'csi'])
def test_applybqsr_with_an_index_both_ways(files, tmp_path, kind):
    got = _both(files, tmp_path, ['applybqsr', '-b', 'IN', '-g', files['sorted_report'], '-s', '--bam-out', '--bam-index', kind, '-o', 'OUT/out.bam'],
                outputs=('out.bam', 'out.bam.' + kind), source='sorted')
    assert len(got[True][0][1]) > 100


def test_recalibrate_kmers_both_ways(files, tmp_path):
    got = _both(files, tmp_path, ['recalibrate', '-b', 'IN', '--kmers', '-k', '15', '--bam-out', '-g', 'OUT/model.grp', '-o', 'OUT/out.bam'],
                outputs=('out.bam', 'model.grp'), source='kmers')
    assert 'kbbq recalibrate: k=15' in got[True][1] and len(got[True][0][0]) > 100000


def test_the_out_of_order_refusal_both_ways(files, tmp_path):
    said = []
    for device in (False, True):
        out = tmp_path / ('%d.bam' % device)
        route, err = _kbbq('applybqsr', '-b', files['bam'], '-g', files['report'], '--bam-out', '--bam-index', '-o', out, device=device, ok=False)
        assert route['route'] == ('device' if device else 'host') and not out.exists() and not (tmp_path / ('%d.bam.bai' % device)).exists()
        said.append(err.strip().split('\n')[-1])
    assert said[0] == said[1] and 'out of coordinate order' in said[0]


def test_a_negative_quality_both_ways(tmp_path):
    """One record, a model that takes it to quality -3: the same ValueError on both routes, and no record in what is left behind."""
    import gzip
    from kbbq import aln
    from kbbq.gatk import applybqsr
    line = '\t'.join(['lonely', '0', 'chr1', '100', '60', '20M', '*', '0', '0', 'ACGT' * 5, 'I' * 20, 'RG:Z:rg0'])
    path = bamwriter.write_bam(tmp_path / 'one.bam', O.sam_text([line]))
    R, Q, S2 = 1, 43, 40
    model = [np.array([2]), np.array([-5]), np.zeros((R, Q), np.int64), np.zeros((R, Q, S2), np.int64), np.zeros((R, Q, 17), np.int64)]
    left = []
    for device in (False, True):
        bam = aln.alignments(str(path), device=device, keep_stream=True)
        assert aln.LAST_RUN['bam_in']['route'] == ('device' if device else 'host')
        kw = dict(resident=applybqsr.device_resident(bam, False)) if device else {}
        out = tmp_path / ('%d.bam' % device)
        with pytest.raises(ValueError, match='alignment 0: a new quality below 0') as err:
            applybqsr.write_bam_file(bam, str(out), lambda w: applybqsr.write_alignments_bam(bam, *model, {'rg0': 0}, w, **kw))
        data = out.read_bytes()
        assert b'lonely' not in (gzip.decompress(data) if data else b'')
        left.append((str(err.value), err.value.read_index, data))
        if device:
            assert bam.batch().stream is None                                         # freed with the writer
    assert left[0] == left[1] and not left[0][2].endswith(bamwriter.bgzf(b'')[-28:])  # not a finished file


def test_what_stays_with_the_reader(files, tmp_path):
    """A file with an `f` tag, @SQ lines in another order, a .sam input, SAM-text output, a launcher's environment, a budget the
    stream does not fit: route host with the variable set, and the bytes of the run without it."""
    rng = np.random.default_rng(9)
    recs = C._many(rng)[:50]
    flt = bamwriter.bgzf(C.raw_image(recs + [C._rec(rng, 'f', tags=C.z(b'RG', b'rg0') + b'XFf\0\0\x80\x3f')] + recs[:5]))
    (tmp_path / 'float.bam').write_bytes(flt)
    (tmp_path / 'order.bam').write_bytes(bamwriter.bgzf(C.sq_reordered()))
    rep = files['report']
    cases = [('float.bam', ['--bam-out'], {}, 'a record the decode and the recode do not vouch for (status 0x20)'),
             ('order.bam', ['--bam-out'], {}, 'the @SQ lines do not name the binary reference list in order'),
             (files['sam'], ['--bam-out'], {}, 'not a BGZF file'),
             (files['bam'], [], {}, 'not asked for'),
             (files['bam'], ['--bam-out'], {'KBBQ_DEVICE_BUDGET': '1M'}, None)]
    for k, (name, opts, env, reason) in enumerate(cases):
        outs = []
        for device in (False, True):
            out = tmp_path / ('%d_%d.out' % (k, device))
            said, err = _kbbq('applybqsr', '-b', tmp_path / name if not os.path.isabs(name) else name, '-g', rep, '-s', *opts, '-o', out,
                              device=device, env=env)
            assert said['route'] == 'host', (name, said)
            if device and reason is not None:
                assert said['fallback'] == reason, said
            if device and reason is None:
                assert said['fallback'].startswith('the record stream does not fit the device budget'), said
            outs.append((out.read_bytes(), err))
        assert outs[0] == outs[1] and len(outs[0][0]) > 1000, name
    # a launcher's environment: --bam-out is refused there as it always was, on both routes alike
    said = []
    for device in (False, True):
        _, err = _kbbq('applybqsr', '-b', files['bam'], '-g', rep, '--bam-out', '-o', tmp_path / 'never.bam', device=device,
                       env={'RANK': '0', 'WORLD_SIZE': '2', 'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': '29517'}, ok=False)
        said.append(err.strip().split('\n')[-1])
    assert said[0] == said[1] and '--bam-out does not run across ranks' in said[0] and not (tmp_path / 'never.bam').exists()
