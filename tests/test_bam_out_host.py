"""--bam-out without a GPU: the host half of the BAM encoder (kbbq_bam_header / _check / _layout / _skeleton) and the host twin of
the assemble kernel (kbbq_bam_assemble) against tests/bamwriter.py, the round trip through the BAM reader, the refusals, the
command line, and kbbq/_bamout.py's BamWriter over the host twin and a zlib stand-in for the deflate call."""
import ctypes
import gzip
import io
import os
import re

import numpy as np
import pytest

import bam_out_cases as C
import bamwriter
from test_bgzf_host import BLOCK, EOF, blocks_of, zlib_blocks


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    """About 60 records, hand-made and random, as a parsed file with its planes."""
    from kbbq import aln
    rng = np.random.default_rng(11)
    lines = C.hand_made(rng) + C.random_records(rng, 20)
    path = tmp_path_factory.mktemp('bamout') / 'a.sam'
    path.write_text(C.sam_text(lines), encoding='latin-1')
    bam = aln.AlignmentFile(str(path))
    seq, out, keep, pitch = C.planes(bam, rng)
    assert 55 <= len(bam) <= 70 and keep.any() and not keep.all()
    return dict(bam=bam, lines=lines, seq=seq, out=out, keep=keep, pitch=pitch)


@pytest.mark.parametrize('set_oq', [False, True])
def test_the_encoder_against_bamwriter(case, set_oq):
    bam = case['bam']
    T = C.rendered(bam, case['out'], case['pitch'], set_oq)
    if set_oq:                                                       # records with and without an OQ tag of their own
        added = [a for a, b in zip(T.split('\n')[len(C.HEADER):], case['lines']) if a != b and a.endswith('\tOQ:Z:' + b.split('\t')[10])]
        assert 10 < len(added) < len(case['lines'])
    records, bad = C.host_stream(bam, case['seq'], case['out'], case['pitch'], set_oq, case['keep'])
    assert bad == -1
    assert C.header_bytes(bam) + records == bamwriter.sam_to_bam_bytes(T)


@pytest.mark.parametrize('set_oq', [False, True])
def test_round_trip_through_the_reader(case, set_oq, tmp_path):
    from kbbq import aln
    bam = case['bam']
    T = C.rendered(bam, case['out'], case['pitch'], set_oq)
    stream = C.header_bytes(bam) + C.host_stream(bam, case['seq'], case['out'], case['pitch'], set_oq, case['keep'])[0]
    path = tmp_path / 'rt.bam'
    path.write_bytes(bamwriter.bgzf(stream))
    back = aln.AlignmentFile(str(path))
    assert list(back.header) == C.HEADER
    want = [ln for ln in T.split('\n') if ln and not ln.startswith('@')]
    assert len(back) == len(want)
    for i, line in enumerate(want):
        fields = [x for x in line.split('\t') if x]                  # (an empty tag field is not a tag)
        if fields[6] == fields[2] != '*':
            fields[6] = '='                                          # (the reader names the record's own reference '=')
        assert back.batch().line(i) == '\t'.join(fields), i


def test_seq_letters_follow_the_stated_map(tmp_path):
    """Lower case like upper case, any other byte 15, the last nibble of an odd length 0."""
    from kbbq import aln
    seq = 'acgtn=mrsvwyhkdb' + 'ACGTN' + 'xX.-*?@[`{~!' + 'u'
    assert len(seq) % 2 == 0
    lines = ['\t'.join(['r%d' % k, '0', 'chr1', '7', '9', '*', '*', '0', '0', s, '*']) for k, s in enumerate((seq, seq[:-1], 'g'))]
    path = tmp_path / 'l.sam'
    path.write_text(C.sam_text(lines))
    bam = aln.AlignmentFile(str(path))
    pitch = 48
    plane = bam.batch().plane(0, pitch)
    records, bad = C.host_stream(bam, plane, np.zeros_like(plane), pitch, False, None)
    code = {c: i for i, c in enumerate('=ACMGRSVTWYHKDBN')}
    at = 0
    for s in (seq, seq[:-1], 'g'):
        head = 36 + 3 + 0
        want = [code.get(c.upper(), 15) for c in s] + [0] * (len(s) % 2)
        packed = records[at + head:at + head + (len(s) + 1) // 2]
        assert [x for b in packed for x in (b >> 4, b & 15)] == want
        assert records[at + head + len(packed):at + head + len(packed) + len(s)] == b'\xff' * len(s)
        at += head + len(packed) + len(s)
    assert at == len(records) and bad == -1


def test_a_quality_below_zero_names_the_lowest_row(case):
    out = case['out'].copy()
    rows = [r for r in range(len(case['bam'])) if not case['keep'][r] and case['bam'].batch().qlen[r] >= 10]
    out[rows[7], 9] = 32
    out[rows[3], 0] = 0
    assert C.host_stream(case['bam'], case['seq'], out, case['pitch'], False, case['keep'])[1] == rows[3]
    kept = int(np.flatnonzero(case['keep'] & (case['bam'].batch().qual_len > 0))[0])
    clean = case['out'].copy()
    clean[kept, 0] = 5                                               # a row the plane is not read for
    assert C.host_stream(case['bam'], case['seq'], clean, case['pitch'], False, case['keep'])[1] == -1


GOOD = '\t'.join(['ok', '0', 'chr1', '100', '60', '4M', '=', '200', '0', 'ACGT', 'IIII', 'RG:Z:rg0'])


def _line(**kw):
    f = dict(zip(('qname', 'flag', 'rname', 'pos', 'mapq', 'cigar', 'rnext', 'pnext', 'tlen', 'seq', 'qual'), GOOD.split('\t')[:11]))
    tags = kw.pop('tags', ['RG:Z:rg0'])
    f.update(kw)
    return '\t'.join(list(f.values()) + tags)


REFUSALS = [
    ('rname', _line(rname='chrX'), 'RNAME is not in @SQ'),
    ('rnext', _line(rnext='chr9'), 'RNEXT is not in @SQ'),
    ('qname', _line(qname='q' * 255), 'QNAME longer than 254'),
    ('ncigar', _line(cigar='1M' * 65536), 'more than 65535 CIGAR operations'),
    ('cigar_op', _line(cigar='4Q'), 'unknown CIGAR operation'),
    ('tag_type', _line(tags=['XX:Q:1']), 'malformed tag'),
    ('tag_short', _line(tags=['RG:Z:rg0', 'X:i:1']), 'malformed tag'),
    ('tag_int', _line(tags=['XI:i:12a']), 'malformed tag'),
    ('tag_char', _line(tags=['XA:A:ab']), 'malformed tag'),
    ('tag_float', _line(tags=['XF:f:one']), 'malformed tag'),
    ('tag_array_type', _line(tags=['XB:B:q,1']), 'malformed tag'),
    ('tag_array_value', _line(tags=['XB:B:c,300']), 'malformed tag'),
    ('int_above', _line(tags=['XI:i:4294967296']), 'integer tag outside int32 and uint32'),
    ('int_below', _line(tags=['XI:i:-2147483649']), 'integer tag outside int32 and uint32'),
    ('seq_star', _line(seq='*', cigar='*'), "SEQ is '*' but QUAL is not"),
]


@pytest.mark.parametrize('name,line,phrase', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_alignment_and_create_no_file(tmp_path, name, line, phrase):
    from kbbq import _bamout, aln
    from kbbq.gatk import applybqsr
    k = 3
    path = tmp_path / 'bad.sam'
    path.write_text(C.sam_text([GOOD] * k + [line] + [GOOD, line]))
    bam = aln.AlignmentFile(str(path))
    with pytest.raises(ValueError, match=r'alignment %d cannot be written as BAM: .*%s' % (k, re.escape(phrase))) as err:
        _bamout.check(bam)
    assert err.value.read_index == k
    _bamout.check(bam, 0, k)                                         # the records before it are fine
    with pytest.raises(ValueError, match='alignment 5 '):
        _bamout.check(bam, k + 1)
    out = tmp_path / 'never.bam'

    def write(writer):
        raise AssertionError('the writer was opened')
    with pytest.raises(ValueError, match='alignment %d ' % k):
        applybqsr.write_bam_file(bam, str(out), write)
    assert not out.exists()


def test_header_without_sn_or_ln_is_refused(tmp_path):
    from kbbq import _native as N
    from kbbq import aln
    for sq in ('@SQ\tLN:5', '@SQ\tSN:a', '@SQ\tSN:a\tLN:5x'):
        path = tmp_path / 'h.sam'
        path.write_text(sq + '\n' + GOOD.replace('chr1', '*') + '\n')
        bam = aln.AlignmentFile(str(path))
        need = ctypes.c_size_t(0)
        with pytest.raises(ValueError, match='@SQ'):
            N.check(N.load().kbbq_bam_header(bam.batch()._native, None, 0, ctypes.byref(need)))


def test_layout_refuses_a_stream_of_two_gib_by_its_size_alone(case):
    """Offsets within a slab are 32 bits; what the descriptors say is checked before a byte is written."""
    from kbbq import _native as N
    bam = case['bam']
    desc, skel, size = C.layout(bam, False, case['keep'])
    assert size < 2 ** 31 and desc.dtype == np.uint32 and desc.shape[1] == 6
    assert int(desc[-1, 4]) + int(desc[-1, 1]) + (int(desc[-1, 3]) + 1) // 2 + int(desc[-1, 3]) + int(desc[-1, 2]) == size
    stream = np.full(size + 128, 0xA5, dtype=np.uint8)
    bad = ctypes.c_int64(-1)
    args = lambda d, cap, carry=0: (N.ptr(skel), skel.nbytes, N.ptr(d), len(d), N.ptr(case['seq']), N.ptr(case['out']), case['pitch'],  # noqa: E731
                                    N.ptr(stream), carry, cap, ctypes.byref(bad))
    lib = N.load()
    for field, value in ((4, 2 ** 32 - 8), (0, 2 ** 32 - 8), (3, case['pitch'] + 1), (1, 2 ** 31), (5, 2)):
        broken = desc.copy()
        broken[5, field] = value
        assert lib.kbbq_bam_assemble(*args(broken, size)) == N.KBBQ_E_ARG and 'row 5' in N.last_error()
    assert lib.kbbq_bam_assemble(*args(desc, size - 1)) == N.KBBQ_E_ARG              # the last record does not fit
    assert lib.kbbq_bam_assemble(*args(desc, size + 63, 64)) == N.KBBQ_E_ARG         # ... nor behind a carry
    assert np.all(stream == 0xA5)
    assert lib.kbbq_bam_assemble(*args(desc, size + 64, 64)) == N.KBBQ_OK
    assert np.all(stream[:64] == 0xA5) and np.all(stream[size + 64:] == 0xA5)
    assert stream[64:size + 64].tobytes() == C.host_stream(bam, case['seq'], case['out'], case['pitch'], False, case['keep'])[0]


# ---------------------------------------------------------------- the writer
@pytest.fixture(scope='module')
def many(tmp_path_factory):
    from kbbq import aln
    rng = np.random.default_rng(23)
    lines = C.random_records(rng, 700, lo=90, hi=150)
    path = tmp_path_factory.mktemp('bamout_many') / 'm.sam'
    path.write_text(C.sam_text(lines))
    bam = aln.AlignmentFile(str(path))
    seq, out, keep, pitch = C.planes(bam, rng)
    return dict(bam=bam, seq=seq, out=out, keep=keep, pitch=pitch)


def _written(many, rows, set_oq=True):
    from kbbq import _bamout
    bam, n = many['bam'], len(many['bam'])
    raw = io.BytesIO()
    with _bamout.BamWriter(raw, deflate=zlib_blocks) as w:
        w.header(bam)
        for first in range(0, n, rows):
            m = min(rows, n - first)
            w.records(bam.batch(), first, m, set_oq, many['keep'][first:first + m], many['seq'][first:first + m],
                      many['out'][first:first + m], many['pitch'])
    assert w.closed and not raw.closed
    return raw.getvalue(), w


def test_the_file_does_not_depend_on_the_slabs(many, monkeypatch):
    stream = bamwriter.sam_to_bam_bytes(C.rendered(many['bam'], many['out'], many['pitch'], True))
    assert len(stream) > 2 * BLOCK and len(stream) % BLOCK
    monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '256')
    whole, w = _written(many, 64)
    assert gzip.decompress(whole) == stream
    assert whole == zlib_blocks(stream) + EOF
    blocks = blocks_of(whole)
    assert [b[4] for b in blocks] == [BLOCK] * (len(stream) // BLOCK) + [len(stream) % BLOCK, 0]
    assert w.stream_bytes == len(stream) and w.file_bytes == len(whole) and w.d2h_bytes == w.file_bytes - 28
    assert 0 < w.h2d_bytes < w.stream_bytes
    assert _written(many, 7)[0] == whole
    assert _written(many, 700)[0] == whole
    monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '1')
    assert _written(many, 7)[0] == whole
    assert _written(many, 64)[0] == whole


def test_a_quality_below_zero_reaches_no_sink(many):
    from kbbq import _bamout
    bam = many['bam']
    out = many['out'].copy()
    row = int(np.flatnonzero(~many['keep'])[40])
    out[row, 3] = 20
    raw = io.BytesIO()
    with pytest.raises(ValueError, match='alignment %d: a new quality below 0' % row) as err:
        with _bamout.BamWriter(raw, deflate=zlib_blocks) as w:
            w.records(bam.batch(), 0, 10, False, many['keep'][:10], many['seq'][:10], out[:10], many['pitch'])
            w.records(bam.batch(), 10, len(bam) - 10, False, many['keep'][10:], many['seq'][10:], out[10:], many['pitch'])
    assert err.value.read_index == row and w.closed
    assert raw.getvalue() == b''                                     # the ten records before it were below a block: still carried


def test_an_empty_file_and_a_text_sink():
    from kbbq import _bamout
    raw = io.BytesIO()
    _bamout.BamWriter(raw, deflate=zlib_blocks).close()
    assert raw.getvalue() == EOF
    for sink in (io.StringIO(), None):
        with pytest.raises(ValueError, match='binary'):
            _bamout.BamWriter(sink, deflate=zlib_blocks)


# ---------------------------------------------------------------- the command line
def _main(monkeypatch, argv, target):
    """The keywords `kbbq <argv>` passes to `target` (module, function name), which is replaced."""
    from kbbq import main, parallel
    seen = {}
    module, name = target

    def fake(*args, **kw):
        seen.update(kw)
        return dict(k=31, min_count=2, reads=0, excluded_reads=0, flagged_bases=0, skipped_bases=0)
    monkeypatch.setattr(module, name, fake)
    monkeypatch.setattr(parallel, 'init_from_env', lambda: (1, 0))
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')
    for var in ('RANK', 'WORLD_SIZE'):
        monkeypatch.delenv(var, raising=False)
    main.main(argv)
    return seen


@pytest.mark.parametrize('given', [False, True])
def test_the_option_goes_down_only_when_given(monkeypatch, tmp_path, given):
    from kbbq import main, recalibrate
    from kbbq.gatk import applybqsr
    flag = ['--bam-out'] if given else []
    seen = _main(monkeypatch, ['applybqsr', '-b', 'x.sam', '-g', 'x.report', '-o', 'out.bam'] + flag, (applybqsr, 'apply_report'))
    assert ('bam_out' in seen) == given and seen['output'] == 'out.bam'
    sam = tmp_path / 'x.sam'
    sam.write_text(C.sam_text([GOOD]))
    monkeypatch.setattr(main._recal, 'check_bam_records', lambda *a, **k: None)
    seen = _main(monkeypatch, ['recalibrate', '-b', str(sam), '--kmers', '-o', str(tmp_path / 'o.x')] + flag, (recalibrate, 'recalibrate_bam'))
    assert ('bam_out' in seen) == given and seen['output'].endswith('o.x')


def test_a_bam_name_is_refused_only_without_the_option(tmp_path):
    from kbbq import recalibrate
    from kbbq.gatk import applybqsr
    with pytest.raises(ValueError, match=r'writes SAM text; BAM output \(x.BAM\) is not supported'):
        applybqsr.apply_report('nowhere.sam', 'nowhere.report', output='x.BAM')
    with pytest.raises(ValueError, match=r'writes SAM text; BAM output \(x.bam\) is not supported'):
        recalibrate.check_bam_kmers('nowhere.sam', None, 'x.bam')
    recalibrate.check_bam_kmers('nowhere.sam', None, 'x.bam', bam_out=True)
    assert not os.path.exists('x.bam')


@pytest.mark.parametrize('argv', [['applybqsr', '-b', 'x.sam', '-g', 'r', '--bam-out', '--bgzf'],
                                  ['recalibrate', '-b', 'x.sam', '--kmers', '--bam-out', '--bgzf'],
                                  ['recalibrate', '-b', 'x.sam', '--bam-out'],
                                  ['recalibrate', '-f', 'a.fq', 'b.fq', '--bam-out'],
                                  ['recalibrate', '-c', 'a.fq', '--bam-out'],
                                  ['bqsr', '-b', 'x.sam', '--kmers', '-g', 'r', '--bam-out']])
def test_argparse_errors(argv, monkeypatch, capsys):
    from kbbq import main, parallel

    def never():
        raise AssertionError('the process group was touched')
    monkeypatch.setattr(parallel, 'init_from_env', never)
    with pytest.raises(SystemExit) as err:
        main.main(argv)
    assert err.value.code == 2
    assert '--bam-out' in capsys.readouterr().err


@pytest.mark.parametrize('argv', [['applybqsr', '-b', 'x.sam', '-g', 'r', '--bam-out', '-o', 'o.bam'],
                                  ['recalibrate', '-b', 'x.sam', '--kmers', '--bam-out', '-o', 'o.bam']])
def test_under_a_launcher_the_option_is_refused_before_the_group(argv, monkeypatch):
    from kbbq import main, parallel
    from kbbq.gatk import applybqsr

    def never():
        raise AssertionError('the process group was joined')
    monkeypatch.setattr(parallel, 'init_from_env', never)
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='SAM text path runs under ranks'):
        main.main(argv)
    with pytest.raises(ValueError, match='SAM text path runs under ranks'):
        applybqsr.apply_report('nowhere.sam', 'nowhere.report', output='o.bam', bam_out=True)
    assert not os.path.exists('o.bam')


def test_the_symbols_are_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'kbbq_hip.h')).read()
    declared = dict(re.findall(r'^int (kbbq_bam_\w+)\(([^;]*)\);', header, flags=re.M))
    assert sorted(declared) == ['kbbq_bam_assemble', 'kbbq_bam_assemble_dev', 'kbbq_bam_check', 'kbbq_bam_header', 'kbbq_bam_layout',
                                'kbbq_bam_skeleton']
    for name, params in declared.items():
        assert hasattr(lib, name)
        assert len(N.PROTOTYPES[name][1]) == params.count(',') + 1, name
    assert ctypes.sizeof(ctypes.c_uint32) * N.BAM_DESC_WORDS == 24
    bad = ctypes.c_int64(5)
    assert lib.kbbq_bam_assemble_dev(None, None, 0, None, 1, None, None, 16, None, 0, 0, ctypes.byref(bad)) == N.KBBQ_E_ARG
    assert bad.value == -1
    assert lib.kbbq_bam_assemble(None, 0, None, 0, None, None, 24, None, 0, 0, ctypes.byref(bad)) == N.KBBQ_E_ARG
    assert 'pitch' in N.last_error()
