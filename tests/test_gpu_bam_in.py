"""BAM input on the GPU: the decode kernel (kbd_decode) against its host twin byte for byte on the cases and slab cuts of
tests/bam_in_cases.py, aln.alignments(device=True) against the host reader attribute by attribute, every case that stays with the
reader, and the two commands -- `bqsr --kmers`, `count -b` -- with KBBQ_GPU_BAM=1 and without it: the same bytes, the same stderr,
the same refusals."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_in_cases as C
import bamwriter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED', 'KBBQ_GPU_BAM', 'KBBQ_STAGE_MB'):
    ENV.pop(_var, None)


def _raw(img):
    return np.frombuffer(img, dtype=np.uint8)


def _pitch_for(n):
    return max(16, (int(n) + 15) // 16 * 16)


def _device(img, scan, pitch, slab_bytes):
    """kbbq._bamin.decode_device's outputs, downloaded, in decode_host's form; every output poisoned first."""
    from kbbq import _bamin as B
    planes, words, cigar, status, _, _ = B.decode_device(_raw(img), scan, pitch, slab_bytes, poison=0xA5)
    out = {p: planes[p].cpu().numpy()[:scan.n] for p in B.PLANES}
    out.update(words=words.cpu().numpy()[:scan.n], cigar=cigar.cpu().numpy().view(np.uint32)[:scan.cig_total], status=status)
    return out


def _same(got, want, what):
    assert got['status'] == want['status'], what
    for key in ('seq', 'qual', 'oq', 'words', 'cigar'):
        assert np.array_equal(got[key], want[key]), (key, what)


@pytest.mark.parametrize('name', list(C.CASES))
def test_kernel_equals_host_twin(name):
    from kbbq import _bamin as B
    img = C.image(name)
    scan = B.Scan(_raw(img))
    full = _pitch_for(max(scan.maxlen, 1))
    cuts = C.slab_cuts(name) if scan.n <= 300 else [None, 1000]
    for pitch, slab_cuts in ((full, cuts), (32 if full != 32 else 16, [None, 1000])):
        for slab_bytes in slab_cuts:
            _same(_device(img, scan, pitch, slab_bytes), B.decode_host(_raw(img), scan, pitch, slab_bytes), (name, pitch, slab_bytes))


@pytest.mark.parametrize('kind', C.CORRUPTIONS)
def test_kernel_equals_host_twin_on_damaged_records(kind):
    from kbbq import _bamin as B
    img, row, bit = C.corrupted(kind)
    scan = B.Scan(_raw(img))
    for pitch in (32, 16):
        for slab_bytes in (None, 1):
            got = _device(img, scan, pitch, slab_bytes)
            assert got['status'] == bit and not got['seq'][row].any() and not got['qual'][row].any() and not got['oq'][row].any()
            _same(got, B.decode_host(_raw(img), scan, pitch, slab_bytes), (kind, pitch, slab_bytes))


def _attributes(got, ref):
    g, r = got.batch(), ref.batch()
    assert g.n == r.n and g.maxlen == r.maxlen and len(got) == len(ref) and list(got.header) == list(ref.header)
    for name in ('flag', 'contig', 'pos', 'pnext', 'tlen', 'qlen', 'ref_span', 'clip', 'cig_off', 'cig_n', 'cigar', 'rg', 'qual_len', 'oq_len'):
        a, b = getattr(g, name), getattr(r, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert g.rg_ids == r.rg_ids and g.contig_names == r.contig_names
    assert np.array_equal(g.adaptor_trim(), r.adaptor_trim()) and g.adaptor_trim().dtype == r.adaptor_trim().dtype
    return g, r


@pytest.mark.parametrize('name', ['hand_made', 'lengths', 'qualities', 'rg300', 'tags', 'cigars', 'trims', 'no_header_text', 'padded_header',
                                  'empty', 'count257'])
def test_alignments_on_the_device_equal_the_reader(name, tmp_path):
    from kbbq import _bamin as B
    from kbbq import aln
    ref, path = C.reader(tmp_path, C.image(name))
    for slab_bytes in (None, 1000):
        got = aln.alignments(path, device=True, slab_bytes=slab_bytes)
        run = aln.LAST_RUN['bam_in']
        assert isinstance(got, aln.DeviceAlignments) and isinstance(got, aln.AlignmentFile), run
        g, r = _attributes(got, ref)
        assert run['route'] == 'device' and run['fallback'] is None and run['records'] == r.n
        assert run['stream_bytes'] <= run['h2d_bytes'] and run['slabs'] == len(B.slabs(B.Scan(_raw(C.image(name))), slab_bytes))
        pitch = _pitch_for(max(r.maxlen, 1))
        for which in range(3):
            assert np.array_equal(g.device_plane(which, pitch).cpu().numpy(), r.plane(which, pitch)), which
            for other in (16, pitch + 16):
                assert np.array_equal(g.plane(which, other), r.plane(which, other)), (which, other)
                assert np.array_equal(g.device_plane(which, other).cpu().numpy(), r.plane(which, other)), (which, other)
            if r.n > 2:
                assert np.array_equal(g.plane(which, pitch, 1, r.n - 2), r.plane(which, pitch, 1, r.n - 2))
    if ref.batch().n:
        assert g.names() == r.names() and g.line(0) == r.line(0) and g._text(0, r.n - 1) == r._text(0, r.n - 1)
        assert str(next(iter(got))) == str(next(iter(ref)))
    only = aln.alignments(path, device=True, planes=('seq',)).batch()                  # a plane that was not kept comes from the reader
    assert np.array_equal(only.device_plane(1, 16).cpu().numpy(), ref.batch().plane(1, 16))


def test_what_stays_with_the_reader(tmp_path, monkeypatch):
    """A flagged file, SAM text, a .sam.gz (BGZF and plain gzip), a damaged image and a launcher's environment: route 'host' with
    the reason, and the reader's batch -- or the reader's error."""
    from kbbq import aln
    monkeypatch.setenv('KBBQ_GPU_BAM', '1')
    for kind in ('qual94', 'rg_tab', 'l_name0'):
        img, _, bit = C.corrupted(kind)
        path = tmp_path / (kind + '.bam')
        path.write_bytes(bamwriter.bgzf(img))
        try:
            want = aln.AlignmentFile(str(path))
        except ValueError as exc:
            with pytest.raises(ValueError) as said:
                aln.alignments(str(path))
            assert str(said.value) == str(exc)
        else:
            got = aln.alignments(str(path))
            assert type(got) is aln.AlignmentFile
            _attributes(got, want)
        run = aln.LAST_RUN['bam_in']
        assert run['route'] == 'host' and run['fallback'] == 'a record the decode does not vouch for (status 0x%x)' % bit
    text = C.sam_text(C.random_records(np.random.default_rng(5), 30))
    sam, bgz, gz = tmp_path / 'x.sam', tmp_path / 'x.sam.gz', tmp_path / 'y.sam.gz'
    sam.write_text(text)
    bgz.write_bytes(bamwriter.bgzf(text.encode()))
    gz.write_bytes(gzip.compress(text.encode()))
    want = aln.AlignmentFile(str(sam))
    for path, reason in ((sam, 'not a BGZF file'), (bgz, 'not a BAM stream'), (gz, 'not a BGZF file')):
        got = aln.alignments(str(path))
        assert type(got) is aln.AlignmentFile and aln.LAST_RUN['bam_in']['route'] == 'host'
        assert aln.LAST_RUN['bam_in']['fallback'] == reason
        _attributes(got, want)
    bad = tmp_path / 'cut.bam'
    bad.write_bytes(bamwriter.bgzf(C.image('hand_made')[:-3]))
    with pytest.raises(ValueError) as said:
        aln.alignments(str(bad))
    assert str(said.value) == '%s: BAM: truncated record' % bad and aln.LAST_RUN['bam_in']['fallback'] == 'scan: BAM: truncated record'
    ref, path = C.reader(tmp_path, C.image('count17'))
    assert isinstance(aln.alignments(path), aln.DeviceAlignments)
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '2')
    got = aln.alignments(path)
    assert type(got) is aln.AlignmentFile and aln.LAST_RUN['bam_in']['fallback'] == 'a rank of a launcher'
    _attributes(got, ref)


# ---- the two commands -----------------------------------------------------------------------------------------------------------------
# a child of its own, as the command line starts: the command, then the route on stdout
CHILD = ('import sys\nfrom kbbq import aln, main\nmain.main(sys.argv[1:])\n'
         'sys.stderr.flush()\nprint("route=%s" % aln.LAST_RUN.get("bam_in", {}).get("route"))\n')


def _kbbq(*argv, device=False):
    env = dict(ENV, KBBQ_GPU_BAM='1') if device else ENV
    r = subprocess.run([sys.executable, '-c', CHILD] + list(argv), capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode().strip(), r.stderr.decode()


@pytest.fixture(scope='module')
def reads(tmp_path_factory):
    """3,000 records of the kind tests/test_gpu_bqsr_kmers.py builds, as SAM and as BAM."""
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('bam_in')
    paths = OQ.synth_bqsr_set(str(d), seed=11, npairs=1500, S=60, contigs=(('chr1', 4000), ('chr2', 3500)))
    paths['bam'] = str(bamwriter.write_bam(d / 'aln.bam', open(paths['sam']).read()))
    paths['dir'] = d
    return paths


@pytest.mark.parametrize('options', [[], ['-u'], ['--mixed-lengths'], ['-F', '0xF00'], ['--kmer-min-qual', '20'],
                                     ['--skip-unresolved', '--passes', '2']], ids=lambda o: ' '.join(o) or 'plain')
def test_bqsr_kmers_both_ways(reads, options, tmp_path):
    out = {}
    for device in (False, True):
        grp = tmp_path / ('%d.grp' % device)
        route, err = _kbbq('bqsr', '--kmers', '-k', '15', '-b', reads['bam'], '-g', str(grp), *options, device=device)
        out[device] = (grp.read_bytes(), err)
        assert route == 'route=%s' % ('device' if device else 'host')
    assert out[True] == out[False] and len(out[True][0]) > 1000 and 'kbbq bqsr: k=15' in out[True][1]


@pytest.mark.parametrize('more', [[], ['-f', 'FASTQ'], ['--kmer-min-qual', '20', '-u']], ids=lambda m: ' '.join(m) or 'plain')
def test_count_both_ways(reads, more, tmp_path):
    """The set's bytes and the stderr line; alone, with a FASTQ beside it, and gated by the OQ tag's qualities."""
    fq = tmp_path / 'extra.fq'
    rng = np.random.default_rng(2)
    fq.write_text(''.join('@q%d\n%s\n+\n%s\n' % (i, ''.join('ACGT'[int(c)] for c in rng.integers(0, 4, 50)), 'I' * 50) for i in range(200)))
    more = [str(fq) if m == 'FASTQ' else m for m in more]
    out = {}
    for device in (False, True):
        path = tmp_path / ('%d.set' % device)
        route, err = _kbbq('count', '-k', '15', '-b', reads['bam'], '-o', str(path), *more, device=device)
        out[device] = (path.read_bytes(), err)
        assert route == 'route=%s' % ('device' if device else 'host')
    assert out[True] == out[False] and 'kbbq count: k=15' in out[True][1] and 'reads=%d' % (3000 + 200 * ('-f' in more)) in out[True][1]


REFUSALS = {
    'no RG': (dict(), lambda f: f[:11] + [t for t in f[11:] if not t.startswith('RG:Z:')]),
    'unknown RG': (dict(), lambda f: f[:11] + ['RG:Z:nowhere' if t.startswith('RG:Z:') else t for t in f[11:]]),
    "QUAL '*'": (dict(), lambda f: f[:10] + ['*'] + f[11:]),
    'missing OQ with -u': (dict(use_oq=True), lambda f: f[:11] + [t for t in f[11:] if not t.startswith('OQ:Z:')]),
    'two lengths': (dict(), lambda f: f[:5] + ['%dM' % (len(f[9]) - 1)] + f[6:9] + [f[9][1:], f[10][1:]] + f[11:]),
    'quality count': (dict(use_oq=True), lambda f: f[:11] + [t[:-2] if t.startswith('OQ:Z:') else t for t in f[11:]]),
    'quality count, mixed': (dict(use_oq=True, mixed_lengths=True), lambda f: f[:11] + [t[:-2] if t.startswith('OQ:Z:') else t for t in f[11:]]),
    'no bases': (dict(use_oq=True, mixed_lengths=True),
                 lambda f: f[:5] + ['*'] + f[6:9] + ['*', '*'] + ['OQ:Z:' if t.startswith('OQ:Z:') else t for t in f[11:]]),
}


@pytest.mark.parametrize('refusal', list(REFUSALS))
def test_every_refusal_is_the_readers(reads, refusal, tmp_path, monkeypatch):
    """The same exception type and message through the BAM with the variable set as from the reader."""
    from kbbq import aln
    from kbbq.gatk import bqsr
    kw, damage = REFUSALS[refusal]
    lines = open(reads['sam']).read().split('\n')
    at = [j for j, ln in enumerate(lines) if ln and not ln.startswith('@')][40]
    lines[at] = '\t'.join(damage(lines[at].split('\t')))
    path = bamwriter.write_bam(tmp_path / 'refused.bam', '\n'.join(lines[:at + 20]))
    said = []
    for device in (False, True):
        if device:
            monkeypatch.setenv('KBBQ_GPU_BAM', '1')
        else:
            monkeypatch.delenv('KBBQ_GPU_BAM', raising=False)
        bam = aln.alignments(path)
        assert aln.LAST_RUN['bam_in']['route'] == ('device' if device else 'host')
        with pytest.raises((KeyError, ValueError)) as exc:
            bqsr.bam_to_kmer_covariates(bam, k=15, **kw)
        said.append((type(exc.value), str(exc.value)))
    assert said[0] == said[1], refusal
