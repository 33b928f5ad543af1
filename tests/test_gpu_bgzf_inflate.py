"""bi_inflate on the MI355X (csrc/kbbq_bgzf_inflate.h) through kbbq_inflate_bgzf_dev, kbbq_inflate_bgzf and the readers.

The members are those of tests/bgzf_inflate_cases.py: the valid ones must come back as the host twin (and zlib) gives them, the
damaged ones -- the fixed list, every entry of which the twin has refused on the CPU and under the sanitizers -- must get the
twin's status and leave every byte of the output buffer as it was.  There is no randomised damage here."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import bgzf_inflate_cases as C
from test_bgzf_inflate_host import twin
from test_gpu_parity import dev                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GAP = 37                                             # sentinel bytes between output ranges: every alignment mod 16 occurs


def inflate_dev(dev, members, lead=0):
    """members: [(payload, isize, crc)].  The payloads end to end behind `lead` bytes (so that they begin at every alignment), the
    output ranges GAP sentinel bytes apart in a buffer of 0xA5.  Returns (status words, the output buffer, the dst offsets)."""
    import torch
    N = dev.N
    src = bytearray(b'\x5a' * lead)
    blocks = (N.BgzfBlock * len(members))()
    dst = GAP
    for b, (payload, isize, crc) in zip(blocks, members):
        b.src, b.csize, b.dst, b.isize, b.crc = len(src), len(payload), dst, isize, crc
        src += payload
        dst += isize + GAP
    d_src = torch.from_numpy(np.frombuffer(bytes(src) + b'\0', dtype=np.uint8).copy()).cuda()
    d_blocks = torch.from_numpy(np.frombuffer(bytes(blocks), dtype=np.uint8).copy()).cuda()
    d_out = torch.full((dst,), 0xA5, dtype=torch.uint8, device='cuda')
    d_status = torch.full((len(members),), -1, dtype=torch.int32, device='cuda')
    N.check(N.load().kbbq_inflate_bgzf_dev(dev.context().handle, N.ptr(d_src), len(src), N.ptr(d_blocks), len(members), N.ptr(d_out),
                                           dst, N.ptr(d_status)))
    return d_status.cpu().numpy(), d_out.cpu().numpy(), [b.dst for b in blocks]


def check_ranges(members, status, out, dsts, texts):
    """Status 0: the text in its range; any other status: the range untouched.  The sentinels between the ranges always."""
    at = 0
    for (payload, isize, crc), st, dst, text in zip(members, status, dsts, texts):
        assert np.all(out[at:dst] == 0xA5), 'sentinel bytes before a range were written'
        got = out[dst:dst + isize]
        if st == 0:
            assert got.tobytes() == text
        else:
            assert np.all(got == 0xA5), 'a refused member wrote to its range'
        at = dst + isize
    assert np.all(out[at:] == 0xA5)


@pytest.mark.parametrize('lead', [0, 5])
def test_the_valid_members_in_one_call(dev, lead):
    """Empty, stored, fixed and dynamic members mixed in one launch, payloads and output ranges at every alignment."""
    members = [(p, len(t), zlib.crc32(t)) for _, t, p in C.valid()]
    texts = [t for _, t, _ in C.valid()]
    status, out, dsts = inflate_dev(dev, members, lead)
    assert [int(s) for s in status] == [twin(*m)[0] for m in members] == [0] * len(members)
    check_ranges(members, status, out, dsts, texts)


def test_the_damaged_members_get_the_twins_status_and_write_nothing(dev):
    """The fixed list between valid members in one launch."""
    good = [(p, len(t), zlib.crc32(t)) for _, t, p in C.valid()[2:5]]
    gtext = [t for _, t, _ in C.valid()[2:5]]
    members, texts = [], []
    for k, (name, payload, isize, crc) in enumerate(C.damaged()):
        members += [good[k % 3], (payload, isize, crc)]
        texts += [gtext[k % 3], None]
    status, out, dsts = inflate_dev(dev, members, lead=3)
    want = [twin(*m)[0] for m in members]
    assert [int(s) for s in status] == want
    assert all(s != 0 for s in want[1::2]) and not any(want[0::2])
    check_ranges(members, status, out, dsts, texts)


def test_a_descriptor_outside_the_buffers_is_refused(dev):
    import torch
    N = dev.N
    name, text, payload = C.valid()[2]
    blocks = (N.BgzfBlock * 3)()
    for b, (src, dst) in zip(blocks, ((0, 0), (1, 0), (0, 1))):          # as it is; the payload, then the text, one byte too far
        b.src, b.csize, b.dst, b.isize, b.crc = src, len(payload), dst, len(text), zlib.crc32(text)
    d_src = torch.from_numpy(np.frombuffer(payload, dtype=np.uint8).copy()).cuda()
    d_blocks = torch.from_numpy(np.frombuffer(bytes(blocks), dtype=np.uint8).copy()).cuda()
    d_out = torch.full((len(text) + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    d_status = torch.full((3,), -1, dtype=torch.int32, device='cuda')
    N.check(N.load().kbbq_inflate_bgzf_dev(dev.context().handle, N.ptr(d_src), len(payload), N.ptr(d_blocks), 3, N.ptr(d_out), len(text),
                                           N.ptr(d_status)))
    assert d_status.cpu().tolist() == [0, N.INFLATE_RANGE, N.INFLATE_RANGE]
    out = d_out.cpu().numpy()
    assert out[:len(text)].tobytes() == text and np.all(out[len(text):] == 0xA5)
    # and the arguments
    lib, h = N.load(), dev.context().handle
    assert lib.kbbq_inflate_bgzf_dev(h, N.ptr(d_src), len(payload), N.ptr(d_blocks), 0, None, 0, None) == N.KBBQ_OK
    assert lib.kbbq_inflate_bgzf_dev(h, N.ptr(d_src), len(payload), None, 1, N.ptr(d_out), 8, N.ptr(d_status)) == N.KBBQ_E_ARG
    assert lib.kbbq_inflate_bgzf_dev(h, N.ptr(d_src), len(payload), d_blocks.data_ptr() + 4, 1, N.ptr(d_out), 8, N.ptr(d_status)) == N.KBBQ_E_ARG
    assert lib.kbbq_inflate_bgzf_dev(h, N.ptr(d_src), len(payload), N.ptr(d_blocks), -1, N.ptr(d_out), 8, N.ptr(d_status)) == N.KBBQ_E_ARG


def _host_route(tmp_path, stream):
    """What the readers give for the stream without the device: (text, None) or (None, the error text)."""
    from kbbq import _native as N
    lib = N.load()
    path = tmp_path / 'stream.gz'
    path.write_bytes(stream)
    saved = os.environ.pop('KBBQ_GPU_INFLATE', None)
    try:
        handle, data, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(0)
        rc = lib.kbbq_text_open(str(path).encode(), ctypes.byref(handle), ctypes.byref(data), ctypes.byref(n))
        if rc != N.KBBQ_OK:
            return None, N.last_error().split(': ', 1)[1]
        try:
            return ctypes.string_at(data, n.value), None
        finally:
            lib.kbbq_text_close(handle)
    finally:
        if saved is not None:
            os.environ['KBBQ_GPU_INFLATE'] = saved


def test_the_host_buffer_call_gives_what_the_readers_host_route_gives(dev, tmp_path):
    """Every damaged member between two valid ones, as a stream: the text of the host route, or its error text; a member with bytes
    behind its last deflate block, which the kernel leaves to the host and the host accepts."""
    from kbbq import _bgzf
    name, text, payload = C.valid()[2]
    ok = C.frame(payload, text)
    for name, bad, isize, crc in C.damaged():
        stream = ok + C.frame(bad, isize=isize, crc=crc) + ok + C.EOF
        want, err = _host_route(tmp_path, stream)
        if err is None:
            assert _bgzf.inflate(stream) == want, name
        else:
            with pytest.raises(ValueError) as exc:
                _bgzf.inflate(stream)
            assert str(exc.value) == err == 'corrupt BGZF block (inflate / CRC mismatch)', name
    stream = ok + C.frame(payload + b'\0\0', text) + ok + C.EOF
    st = {}
    assert _bgzf.inflate(stream, st) == _host_route(tmp_path, stream)[0] == 3 * text
    assert st['device_blocks'] == 3 and st['host_blocks'] == 1
    with pytest.raises(ValueError):
        _bgzf.inflate(zlib.compress(b'not BGZF'))
    assert _bgzf.inflate(b'') == b'' and _bgzf.inflate(C.EOF) == b''


def test_more_members_than_workgroups(dev):
    """1,500 members of 100 bytes: every workgroup walks several; through the device call and through the host-buffer call."""
    from kbbq import _bgzf
    text = C.fastq_like(150000, seed=8)
    pieces = [text[i:i + 100] for i in range(0, len(text), 100)]
    assert len(pieces) == 1500 > dev.context().compute_units
    members = [(C.raw(p, 6), len(p), zlib.crc32(p)) for p in pieces]
    status, out, dsts = inflate_dev(dev, members)
    assert not status.any()
    check_ranges(members, status, out, dsts, pieces)
    st = {}
    assert _bgzf.inflate(b''.join(C.frame(m[0], p) for m, p in zip(members, pieces)) + C.EOF, st) == text
    assert st['device_blocks'] == 1501 and st['host_blocks'] == 0 and st['bytes_down'] >= len(text)


def test_slab_boundaries_between_and_inside_members(dev, monkeypatch):
    """KBBQ_STAGE_MB=1 holds 7 members a slab: the valid members three times over are some ten slabs of whole members, whatever
    their sizes -- the byte budget falls inside members, the slabs end between them."""
    from kbbq import _bgzf
    monkeypatch.setenv('KBBQ_STAGE_MB', '1')
    members = [(t, p) for _, t, p in C.valid()] * 3
    stream = b''.join(C.frame(p, t) for t, p in members)
    st = {}
    assert _bgzf.inflate(stream, st) == b''.join(t for t, _ in members)
    assert st['device_blocks'] == len(members) > 7 * 8 and st['host_blocks'] == 0
    assert st['bytes_up'] >= sum(len(p) for _, p in members)


def test_round_trip_of_the_projects_own_writer(dev):
    """kbbq_bgzf_deflate_dev on 3 x 65280 + 17 bytes of FASTQ-like text, then bi_inflate: the text."""
    import torch
    from kbbq import _bgzf
    N = dev.N
    lib, ctx = N.load(), dev.context()
    text = C.fastq_like(3 * 65280 + 17, seed=12)
    n, nb = len(text), 4
    bound = int(lib.kbbq_bgzf_bound(n, 65280))
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    d_blocks = torch.zeros(nb * N.BGZF_SLOT, dtype=torch.uint8, device='cuda')
    d_sizes = torch.zeros(nb, dtype=torch.int32, device='cuda')
    d_packed = torch.zeros(bound, dtype=torch.uint8, device='cuda')
    total = ctypes.c_size_t(0)
    N.check(lib.kbbq_bgzf_deflate_dev(ctx.handle, N.ptr(d_text), n, 65280, N.ptr(d_blocks), N.ptr(d_sizes), N.ptr(d_packed), ctypes.byref(total)))
    packed = d_packed.cpu().numpy()[:total.value].tobytes()
    st = {}
    assert _bgzf.inflate(packed + C.EOF, st) == text
    assert st['device_blocks'] == 5 and st['host_blocks'] == 0


# ---------------------------------------------------------------- the readers
@pytest.fixture
def registered(dev):
    """The readers know the context (_device.context() registers one when it creates it; a test before may have taken it back)."""
    N = dev.N
    N.check(N.load().kbbq_inflate_use_ctx(dev.context().handle))


def _bgzip(path, block=20000):
    data = open(path, 'rb').read()
    with open(path + '.gz', 'wb') as fh:
        fh.write(b''.join(C.frame(C.raw(data[i:i + block]), data[i:i + block]) for i in range(0, len(data), block)) + C.EOF)
    return path + '.gz'


def test_recalibrate_reads_a_bgzf_pair_through_the_device(dev, registered, oracle, tmp_path, monkeypatch, capsys):
    from kbbq import _bgzf, _trace, recalibrate
    n, R = 2000, 2
    seq, cseq, qual, meta = oracle.synth(0, n, n, 11, nrg=R)
    names = oracle.synth_names(0, n, R, with_rg=True)
    fa, fb = str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')
    oracle.write_fastq(fa, names, seq, qual, meta)
    oracle.write_fastq(fb, names, cseq, qual, meta)
    za, zb = _bgzip(fa), _bgzip(fb)
    out = {}
    before = _bgzf.inflate_stats()
    for mode, files, env in (('plain', [fa, fb], None), ('host', [za, zb], '0'), ('unset', [za, zb], None), ('device', [za, zb], '1')):
        monkeypatch.setenv('KBBQ_GPU_INFLATE_MIN_BYTES', '0')
        if env is None:
            monkeypatch.delenv('KBBQ_GPU_INFLATE', raising=False)
        else:
            monkeypatch.setenv('KBBQ_GPU_INFLATE', env)
        if mode == 'device':
            assert _bgzf.inflate_stats() == before                       # nothing went to the device unasked
        o = str(tmp_path / (mode + '.out.fq'))
        recalibrate.recalibrate_fastq(files, infer_rg=True, output=o)
        out[mode] = open(o, 'rb').read()
    assert out['device'] == out['plain'] == out['host'] == out['unset'] and len(out['plain']) > 100 * n
    after = _bgzf.inflate_stats()
    blocks = sum((os.path.getsize(p) + 19999) // 20000 + 1 for p in (fa, fb))
    assert after['device_blocks'] - before['device_blocks'] == blocks and after['host_blocks'] == before['host_blocks']
    # the stage report names the device inflate and its fallback count
    monkeypatch.setattr(_trace, 'ON', True)
    _trace._acc['test'] = (0.0, 1)
    capsys.readouterr()
    _trace.report()
    err = capsys.readouterr().err
    assert 'kbbq inflate: %d BGZF blocks inflated on the device, %d redone on the host' % (after['device_blocks'], after['host_blocks']) in err
    # below the threshold the reader stays on the host
    monkeypatch.setenv('KBBQ_GPU_INFLATE_MIN_BYTES', str(1 << 30))
    recalibrate.recalibrate_fastq([za, zb], infer_rg=True, output=str(tmp_path / 'small.out.fq'))
    assert open(str(tmp_path / 'small.out.fq'), 'rb').read() == out['plain'] and _bgzf.inflate_stats() == after


def test_applybqsr_reads_a_bam_through_the_device(dev, registered, tmp_path, monkeypatch):
    import bamwriter
    from kbbq import _bgzf, aln
    from kbbq.gatk import applybqsr
    from test_gpu_applybqsr import _random_model, _random_sam
    sam = _random_sam(tmp_path / 'r.sam', seed=21)
    bam = str(bamwriter.write_bam(tmp_path / 'r.bam', open(sam).read()))
    model, rg_to_int = _random_model(7, 3, 40), {'g0': 0, 'g1': 1, 'g2': 2}
    monkeypatch.setenv('KBBQ_GPU_INFLATE_MIN_BYTES', '0')
    got = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('KBBQ_GPU_INFLATE', mode)
        before = _bgzf.inflate_stats()
        f = aln.AlignmentFile(bam)
        got[mode] = applybqsr.recalibrate_alignments(f, *model, rg_to_int)
        after = _bgzf.inflate_stats()
        if mode == '1':
            assert after['device_blocks'] > before['device_blocks'] and after['host_blocks'] == before['host_blocks']
        else:
            assert after == before
    assert np.array_equal(got['0'][0], got['1'][0]) and np.array_equal(got['0'][1], got['1'][1]) and got['0'][0].size > 1000
