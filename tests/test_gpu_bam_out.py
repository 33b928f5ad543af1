"""--bam-out on the MI355X: the assemble kernel (kbbq_bam_assemble_dev, csrc/kbbq_bam_out.h) against its host twin on synthetic
descriptors -- every destination residue, every path of a segment, canaries around the stream -- and the two commands end to end:
the inflated file is tests/bamwriter.py's encoding of the SAM text the same command writes without the option."""
import ctypes
import gzip
import os
import sys

import numpy as np
import pytest

import bam_out_cases as C
import bamwriter
from test_bgzf_host import BLOCK, EOF, blocks_of

pytestmark = pytest.mark.gpu

CANARY = 64


# ---------------------------------------------------------------- the kernel against its host twin
def _synthetic(n, pitch, seed):
    """Descriptors, skeleton and planes of n made-up records: lengths at the edges of the 16-byte pieces and of the row, heads
    and tails (0 and odd among them) that move the SEQ and QUAL destinations over every residue mod 16, the three QUAL kinds mixed."""
    rng = np.random.default_rng(seed)
    lengths = [x for x in (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, pitch - 1, pitch) if x <= pitch]
    tails = (0, 1, 3, 8, 21, 40, 5, 0, 17)
    desc = np.zeros((n, 6), dtype=np.uint32)
    skel_at = stream_at = 0
    for r in range(n):
        L = lengths[(r + r // len(lengths)) % len(lengths)]
        head, tail, src = 36 + (r * 7 + r // 7) % 23, tails[r % len(tails)], 1 if r % 3 == 1 else 0
        desc[r] = (skel_at, head, tail, L, stream_at, src)
        skel_at += head + (L if src else 0) + tail
        stream_at += head + (L + 1) // 2 + L + tail
    skel = rng.integers(0, 256, max(skel_at, 1)).astype(np.uint8)
    for r in range(n):                                               # every other skeleton QUAL is a '*' one
        if desc[r, 5] and r % 2:
            at = int(desc[r, 0] + desc[r, 1])
            skel[at:at + int(desc[r, 3])] = 0xFF
    seq = rng.choice(np.frombuffer(b'ACGTNacgtn=MRSVWYHKDBxX.*\x00\xff', dtype=np.uint8), (n, pitch))
    out = rng.integers(33, 127, (n, pitch)).astype(np.uint8)
    return desc, skel[:skel_at], seq, out, stream_at


def _host(desc, skel, seq, out, pitch, size, carry):
    from kbbq import _native as N
    buf = np.full(CANARY + carry + size + CANARY, 0xA5, dtype=np.uint8)
    bad = ctypes.c_int64(-7)
    N.check(N.load().kbbq_bam_assemble(N.ptr(skel), skel.nbytes, N.ptr(desc), len(desc), N.ptr(seq), N.ptr(out), pitch,
                                       ctypes.c_void_p(buf.ctypes.data + CANARY), carry, carry + size, ctypes.byref(bad)))
    return buf, int(bad.value)


def _device(desc, skel, seq, out, pitch, size, carry):
    import torch
    from kbbq import _device as dev
    from kbbq import _native as N
    ctx = dev.context()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    d_skel, d_desc, d_seq, d_out = up(skel if skel.size else np.zeros(1, np.uint8)), up(desc.view(np.int32)), up(seq), up(out)
    d_buf = torch.full((CANARY + carry + size + CANARY,), 0xA5, dtype=torch.uint8, device='cuda')
    bad = ctypes.c_int64(-7)
    N.check(N.load().kbbq_bam_assemble_dev(ctx.handle, N.ptr(d_skel), skel.nbytes, N.ptr(d_desc), len(desc), N.ptr(d_seq), N.ptr(d_out),
                                           pitch, N.ptr(d_buf.data_ptr() + CANARY), carry, carry + size, ctypes.byref(bad)))
    return d_buf.cpu().numpy(), int(bad.value)


@pytest.mark.parametrize('pitch', [16, 48, 4112])
@pytest.mark.parametrize('n', [1, 64, 65, 257])
def test_the_kernel_against_its_host_twin(n, pitch):
    desc, skel, seq, out, size = _synthetic(n, pitch, seed=n + pitch)
    if n >= 64:                    # the destinations take every residue mod 16 -- at 257 records among those with 16-byte pieces alone
        seq_at = (desc[:, 4] + desc[:, 1]) % 16
        qual_at = (desc[:, 4] + desc[:, 1] + (desc[:, 3] + 1) // 2) % 16
        long_ = desc[:, 3] >= (min(33, pitch) if n == 257 else 1)
        assert set(seq_at[long_]) == set(range(16)) == set(qual_at[long_]) and set((desc[:, 4] % 16)) == set(range(16))
        assert {0, 1} <= set(desc[:, 2]) and {0, 1} == set(desc[:, 5])
    for carry in (0, 37):
        want, bad_h = _host(desc, skel, seq, out, pitch, size, carry)
        got, bad_d = _device(desc, skel, seq, out, pitch, size, carry)
        assert bad_h == bad_d == -1
        assert np.all(want[:CANARY + carry] == 0xA5) and np.all(want[CANARY + carry + size:] == 0xA5)
        assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0]) - CANARY - carry
        # ... and the host twin is what the fields say (one record spelled out)
        r = n - 1
        at = CANARY + carry + int(desc[r, 4])
        head, tail, L = int(desc[r, 1]), int(desc[r, 2]), int(desc[r, 3])
        assert want[at:at + head].tobytes() == skel[int(desc[r, 0]):int(desc[r, 0]) + head].tobytes()
        if not desc[r, 5]:
            assert np.array_equal(want[at + head + (L + 1) // 2:at + head + (L + 1) // 2 + L], out[r, :L] - 33)
        assert at + head + (L + 1) // 2 + L + tail == CANARY + carry + size


def test_the_bad_quality_word_is_the_lowest_row():
    n, pitch = 257, 48
    desc, skel, seq, out, size = _synthetic(n, pitch, seed=3)
    plane_rows = [r for r in range(n) if not desc[r, 5] and desc[r, 3] >= 33]
    kept_rows = [r for r in range(n) if desc[r, 5] and desc[r, 3] >= 1]
    out[kept_rows[0], 0] = 1                                         # a row whose QUAL is the skeleton's: the plane is not read
    assert _device(desc, skel, seq, out, pitch, size, 0)[1] == -1
    for rows_cols in ([(plane_rows[-1], 32)], [(plane_rows[9], 0), (plane_rows[4], 20), (plane_rows[30], 5)], [(plane_rows[2], 16)]):
        bad = out.copy()
        for r, c in rows_cols:
            bad[r, c] = 32
        want = min(r for r, _ in rows_cols)
        assert _host(desc, skel, seq, bad, pitch, size, 0)[1] == want
        assert _device(desc, skel, seq, bad, pitch, size, 5)[1] == want
    past = out.copy()
    r = next(r for r in plane_rows if desc[r, 3] == 33)
    past[r, 33:] = 0                                                 # behind the record's length: not its quality
    assert _device(desc, skel, seq, past, pitch, size, 0)[1] == -1


def test_a_descriptor_out_of_bounds_writes_nothing():
    from kbbq import _native as N
    n, pitch = 65, 48
    desc, skel, seq, out, size = _synthetic(n, pitch, seed=4)
    broken = desc.copy()
    broken[40, 4] = size                                             # the record would begin where the stream ends
    with pytest.raises(ValueError, match='row 40'):
        _device(broken, skel, seq, out, pitch, size, 0)
    broken = desc.copy()
    broken[7, 3] = pitch + 1
    with pytest.raises(ValueError, match='row 7'):
        _device(broken, skel, seq, out, pitch, size, 0)
    assert N.KBBQ_E_ARG == -4


# ---------------------------------------------------------------- end to end
@pytest.fixture
def kbbq(monkeypatch, capfdbinary):
    """The command line in this process: main.main(argv) -> (stdout bytes, stderr text)."""
    from kbbq import main
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)

    def run(*argv):
        capfdbinary.readouterr()
        main.main([str(a) for a in argv])
        sys.stdout.flush()
        sys.stderr.flush()
        out, err = capfdbinary.readouterr()
        return out, err.decode()
    return run


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """Random records of lengths 1..70 over three read groups, 15 % without OQ, some with QUAL '*', as SAM and as BAM; a report."""
    from kbbq.gatk import bqsr
    d = tmp_path_factory.mktemp('bam_out_e2e')
    rng = np.random.default_rng(77)
    text = C.sam_text(C.random_records(rng, 640))
    (d / 'in.sam').write_text(text)
    bamwriter.write_bam(d / 'in.bam', text)
    R, Q, S2 = 3, 43, 140
    q_total = rng.integers(0, 5000, (R, Q))
    q_errs = (q_total * rng.uniform(0, 0.05, (R, Q))).astype(np.int64)
    pos_total = rng.integers(0, 200, (R, Q, S2))
    pos_errs = (pos_total * rng.uniform(0, 0.1, (R, Q, S2))).astype(np.int64)
    dn_total = rng.integers(0, 800, (R, Q, 16))
    dn_errs = (dn_total * rng.uniform(0, 0.1, (R, Q, 16))).astype(np.int64)
    report = bqsr.vectors_to_report(np.zeros(R), q_errs.sum(1), q_total.sum(1), q_errs, q_total, pos_errs, pos_total, dn_errs, dn_total,
                                    ['pu0', 'pu1', 'pu2'])
    (d / 'model.grp').write_text(str(report))
    return dict(dir=d, sam=str(d / 'in.sam'), bam=str(d / 'in.bam'), report=str(d / 'model.grp'), text=text)


OPTIONS = [(), ('-u',), ('-s',), ('-u', '-s'), ('--static-quantized-quals', '10,20,30')]


@pytest.mark.parametrize('opts', OPTIONS, ids=['plain', 'u', 's', 'u-s', 'quantized'])
@pytest.mark.parametrize('source', ['sam', 'bam'])
def test_applybqsr_writes_the_stream_its_sam_text_defines(files, kbbq, tmp_path, source, opts):
    from kbbq.gatk import applybqsr
    T, err_sam = kbbq('applybqsr', '-b', files[source], '-g', files['report'], *opts)
    stream = bamwriter.sam_to_bam_bytes(T.decode('latin-1'))
    assert len(stream) > BLOCK and T.count(b'\n') == 640 + len(C.HEADER)
    out = tmp_path / 'out.anything'
    said = kbbq('applybqsr', '-b', files[source], '-g', files['report'], *opts, '--bam-out', '-o', out)
    assert said == (b'', err_sam)                                    # stderr is what it was
    data = out.read_bytes()
    assert gzip.decompress(data) == stream
    counters = dict(applybqsr.LAST_RUN['bam_out'])
    assert counters['file_bytes'] == len(data) and counters['stream_bytes'] == len(stream)
    assert counters['d2h_bytes'] == counters['file_bytes'] - 28 and 0 < counters['h2d_bytes'] < len(stream)
    to_stdout, err = kbbq('applybqsr', '-b', files[source], '-g', files['report'], *opts, '--bam-out')
    assert to_stdout == data and err == err_sam
    if opts in ((), ('-s',)):                                        # the changed qualities are in it, and the OQ tags -s adds
        assert T != files['text'].encode() and (b'OQ:Z:' in T)
        assert (T.count(b'OQ:Z:') > files['text'].count('OQ:Z:')) == (opts == ('-s',))


def test_block_structure_and_slab_independence(files, kbbq, tmp_path, monkeypatch):
    from kbbq.gatk import applybqsr
    out = tmp_path / 'a.bam'
    kbbq('applybqsr', '-b', files['sam'], '-g', files['report'], '-s', '--bam-out', '-o', out)
    data = out.read_bytes()
    blocks = blocks_of(data)                                         # (every member's header, 'BC' and BSIZE are checked there)
    sizes = [b[4] for b in blocks]
    assert len(blocks) >= 3 and all(s == BLOCK for s in sizes[:-2]) and 0 < sizes[-2] <= BLOCK and sizes[-1] == 0
    assert data.endswith(EOF)
    for off, size, payload, crc, isize in blocks:
        assert len(gzip.decompress(data[off:off + size])) == isize
    monkeypatch.setattr(applybqsr, '_ROWS', 64)                      # ten slabs: records and slabs straddle the cuts
    again = tmp_path / 'b.bam'
    kbbq('applybqsr', '-b', files['sam'], '-g', files['report'], '-s', '--bam-out', '-o', again)
    assert again.read_bytes() == data
    monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '1')
    kbbq('applybqsr', '-b', files['sam'], '-g', files['report'], '-s', '--bam-out', '-o', again)
    assert again.read_bytes() == data
    # ... and the reader takes the file back: the records of the SAM output
    from kbbq import aln
    T, _ = kbbq('applybqsr', '-b', files['sam'], '-g', files['report'], '-s')
    back = aln.AlignmentFile(str(out))
    want = [ln for ln in T.decode('latin-1').split('\n') if ln and not ln.startswith('@')]
    assert [back.batch().line(i) for i in range(len(back))] == want


@pytest.fixture(scope='module')
def uniform(tmp_path_factory):
    """test_gpu_recalibrate_bam's input (records of one length, as `recalibrate -b --kmers` takes them): as written, every record
    with an OQ tag (what -u needs), and with every other tag removed."""
    import kmer_bqsr_model as B
    import oracle_bqsr as OQ
    from test_gpu_recalibrate_bam import _without_oq
    d = tmp_path_factory.mktemp('bam_out_kmers')
    texts = dict(all=open(OQ.synth_bqsr_set(str(d), **B.FIXTURE)['sam']).read())
    texts['half'] = _without_oq(texts['all'], lambda i: i % 2 == 0)
    paths = {}
    for name, text in texts.items():
        (d / (name + '.sam')).write_text(text)
        paths[name, 'sam'], paths[name, 'bam'] = str(d / (name + '.sam')), bamwriter.write_bam(d / (name + '.bam'), text)
    return paths


@pytest.mark.parametrize('oq,opts', [('half', ()), ('half', ('-s',)), ('all', ('-u', '-s'))], ids=['plain', 's', 'u-s'])
@pytest.mark.parametrize('source', ['sam', 'bam'])
def test_recalibrate_kmers_writes_the_same_stream_and_report(uniform, kbbq, tmp_path, source, oq, opts):
    from kbbq import recalibrate
    k = ('-k', '15')
    uniform = {source: uniform[oq, source]}
    T, err_sam = kbbq('recalibrate', '-b', uniform[source], '--kmers', *k, *opts, '-g', tmp_path / 'sam.grp')
    stream = bamwriter.sam_to_bam_bytes(T.decode('latin-1'))
    out = tmp_path / 'out.bam'
    said = kbbq('recalibrate', '-b', uniform[source], '--kmers', *k, *opts, '--bam-out', '-g', tmp_path / 'bam.grp', '-o', out)
    assert said == (b'', err_sam) and err_sam.startswith('kbbq recalibrate: k=15')
    assert gzip.decompress(out.read_bytes()) == stream
    assert (tmp_path / 'bam.grp').read_bytes() == (tmp_path / 'sam.grp').read_bytes()
    # the resident planes were read where they lay: no plane went up for the BAM
    assert recalibrate.LAST_RUN['aligned']['alignments'] == 600
    to_stdout, _ = kbbq('recalibrate', '-b', uniform[source], '--kmers', *k, *opts, '--bam-out')
    assert to_stdout == out.read_bytes()


def test_the_command_as_a_process_of_its_own(uniform, tmp_path):
    """`recalibrate -b --kmers` on one GPU imports no torch: the writer's buffers then come from the library's own allocator
    (kbbq/_hipmem.py).  The same stream."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, 'kbbq-py_amd'))
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS'):
        env.pop(var, None)
    base = [sys.executable, '-m', 'kbbq.main', 'recalibrate', '-b', uniform['half', 'bam'], '--kmers', '-k', '15', '-s']
    plain = subprocess.run(base, env=env, capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()
    out = tmp_path / 'p.bam'
    made = subprocess.run(base + ['--bam-out', '-o', str(out)], env=env, capture_output=True, timeout=120)
    assert made.returncode == 0 and made.stdout == b'' and made.stderr == plain.stderr, made.stderr.decode()
    assert gzip.decompress(out.read_bytes()) == bamwriter.sam_to_bam_bytes(plain.stdout.decode('latin-1'))


def test_a_negative_quality_is_refused_with_its_index(tmp_path):
    """One record, a model that takes it to quality -3: SAM text holds the character, BAM does not."""
    from kbbq import _bamout, aln
    from kbbq.gatk import applybqsr
    line = '\t'.join(['lonely', '0', 'chr1', '100', '60', '20M', '*', '0', '0', 'ACGT' * 5, 'I' * 20, 'RG:Z:rg0'])
    path = tmp_path / 'one.sam'
    path.write_text(C.sam_text([line]))
    bam = aln.AlignmentFile(str(path))
    R, Q, S2 = 1, 43, 40
    model = [np.array([2]), np.array([-5]), np.zeros((R, Q), np.int64), np.zeros((R, Q, S2), np.int64), np.zeros((R, Q, 17), np.int64)]
    sam = tmp_path / 'one.out.sam'
    with open(sam, 'wb') as sink:
        applybqsr.write_alignments(bam, *model, {'rg0': 0}, sink)
    assert sam.read_text().split('\n')[len(C.HEADER)].split('\t')[10] == chr(33 - 3) * 20
    out = tmp_path / 'one.bam'
    with pytest.raises(ValueError, match='alignment 0: a new quality below 0') as err:
        applybqsr.write_bam_file(bam, str(out), lambda w: applybqsr.write_alignments_bam(bam, *model, {'rg0': 0}, w))
    assert err.value.read_index == 0
    data = out.read_bytes()
    assert b'lonely' not in (gzip.decompress(data) if data else b'')
    assert not data.endswith(EOF)                                    # not a finished file either
    assert isinstance(_bamout.EOF, bytes)
