"""--bgzf without a GPU: kbbq/_bgzf.py's BgzfWriter over a zlib stand-in for the native call (the cut of the stream, the header
bytes, BSIZE, the EOF block, empty input, a text-only sink), the option on the three commands' parsers and the keyword that
goes down only when it is given, and the C ABI: header, prototypes and exported symbols in step, the calls that need no device."""
import ctypes
import gzip
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 65280
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
HEAD = bytes.fromhex('1f8b08040000000000ff060042430200')


def zlib_blocks(text):
    """What the native call returns for `text`, made by zlib: BGZF blocks of the 65280-byte pieces."""
    text = bytes(text)
    out = []
    for lo in range(0, len(text), BLOCK):
        piece = text[lo:lo + BLOCK]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        payload = c.compress(piece) + c.flush()
        out.append(HEAD + struct.pack('<H', 18 + len(payload) + 8 - 1) + payload + struct.pack('<II', zlib.crc32(piece), len(piece)))
    return b''.join(out)


def blocks_of(data):
    """[(offset, BSIZE, payload, crc, isize)] of a BGZF file, every header checked."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 16] == HEAD, at
        size = struct.unpack_from('<H', data, at + 16)[0] + 1
        crc, isize = struct.unpack_from('<II', data, at + size - 8)
        out.append((at, size, data[at + 18:at + size - 8], crc, isize))
        at += size
    assert at == len(data)
    return out


def written(text, piece, slab_blocks=None, monkeypatch=None):
    from kbbq import _bgzf
    if slab_blocks is not None:
        monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', str(slab_blocks))
    raw = io.BytesIO()
    w = _bgzf.BgzfWriter(raw, deflate=zlib_blocks)
    for lo in range(0, len(text), piece or max(len(text), 1)):
        assert w.write(text[lo:lo + (piece or len(text))]) == len(text[lo:lo + (piece or len(text))])
    w.close()
    assert w.closed and not raw.closed
    assert w.text_bytes == len(text) and w.file_bytes == len(raw.getvalue())
    return raw.getvalue()


@pytest.fixture(scope='module')
def text():
    rng = np.random.default_rng(5)
    words = [b'@read', b'ACGT', b'GATTACA', b'+', b'FFFF:FFF', b'\n']
    return b''.join(words[i] for i in rng.integers(0, len(words), 60000))[:3 * BLOCK + 1234]


def test_the_file_is_a_function_of_the_text_alone(text, monkeypatch):
    whole = written(text, None, 2, monkeypatch)
    assert gzip.decompress(whole) == text
    assert whole == zlib_blocks(text) + EOF
    for piece in (1, 7, 65279, 65280, 65281):
        assert written(text, piece, 2, monkeypatch) == whole, piece
    assert written(text, 65281, 1, monkeypatch) == whole             # a slab of one block
    assert written(text, 4096) == whole                              # the default slab: everything goes out in close()


def test_header_bsize_and_eof(text, monkeypatch):
    data = written(text, 50000, 2, monkeypatch)
    blocks = blocks_of(data)
    assert [b[4] for b in blocks] == [BLOCK, BLOCK, BLOCK, 1234, 0]
    at = 0
    for off, size, payload, crc, isize in blocks[:-1]:
        piece = text[at:at + isize]
        assert zlib.decompress(payload, -15) == piece and crc == zlib.crc32(piece)
        assert gzip.decompress(data[off:off + size]) == piece          # every block is a gzip file of its own
        at += isize
    off, size, payload, crc, isize = blocks[-1]
    assert data[off:] == EOF and size == 28 and crc == 0 and zlib.decompress(payload, -15) == b''


def test_empty_input_is_the_eof_block():
    assert written(b'', None) == EOF
    assert gzip.decompress(EOF) == b''


def test_flush_keeps_the_cut_and_close_is_final(text, monkeypatch):
    from kbbq import _bgzf
    monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '1')
    raw = io.BytesIO()
    with _bgzf.BgzfWriter(raw, deflate=zlib_blocks) as w:
        w.write(text[:100])
        w.flush()
        assert raw.getvalue() == b''                                 # a flush does not cut a block short
        w.write(text[100:BLOCK + 5])
        w.flush()
        assert gzip.decompress(raw.getvalue()) == text[:BLOCK]        # ... and waits for the full slabs on their way
        with pytest.raises(io.UnsupportedOperation):
            w.fileno()
        w.write(text[BLOCK + 5:])
    assert raw.getvalue() == zlib_blocks(text) + EOF
    w.close()                                                        # again: nothing more
    assert raw.getvalue() == zlib_blocks(text) + EOF
    with pytest.raises(ValueError):
        w.write(b'x')


def test_an_error_of_the_worker_reaches_the_caller(monkeypatch):
    from kbbq import _bgzf
    monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '1')

    def broken(_):
        raise RuntimeError('no device')
    w = _bgzf.BgzfWriter(io.BytesIO(), deflate=broken)
    w.write(b'a' * (3 * BLOCK))
    with pytest.raises(RuntimeError, match='no device'):
        w.close()
    assert w.closed


def test_a_text_only_sink_is_refused(monkeypatch):
    from kbbq import _bgzf
    for sink in (io.StringIO(), None):
        with pytest.raises(ValueError, match='binary'):
            _bgzf.BgzfWriter(sink, deflate=zlib_blocks)
    monkeypatch.setattr('sys.stdout', io.StringIO())                 # a stdout without .buffer
    with pytest.raises(ValueError, match='binary'):
        _bgzf.stdout_sink()
    with pytest.raises(ValueError, match='binary'):
        with _bgzf.output(True):
            _bgzf.write_text(io.StringIO(), '@r\nA\n+\nF\n')


def test_the_sinks_follow_the_option(tmp_path, monkeypatch):
    from kbbq import _bgzf
    monkeypatch.setattr(_bgzf, '_GpuDeflate', lambda nbytes: _bgzf._CallDeflate(zlib_blocks, nbytes))
    plain = _bgzf.open_sink(str(tmp_path / 'a.gz'))                   # no suffix detection: plain without the option
    assert not isinstance(plain, _bgzf.BgzfWriter)
    with plain:
        plain.write(b'text\n')
    assert (tmp_path / 'a.gz').read_bytes() == b'text\n'

    @_bgzf.option
    def command(path, body):
        assert _bgzf.enabled() == want
        inner(path, body)                                            # an inner entry point without the keyword keeps the choice
        return 7

    @_bgzf.option
    def inner(path, body):
        assert _bgzf.enabled() == want
        with _bgzf.open_sink(path) as sink:
            sink.write(body)
    for want in (False, True):
        p = str(tmp_path / ('out%d' % want))
        assert command(p, b'abc\n', **({'bgzf': True} if want else {})) == 7
        assert not _bgzf.enabled()
        data = open(p, 'rb').read()
        assert data == (zlib_blocks(b'abc\n') + EOF if want else b'abc\n')
    with _bgzf.output(True):
        _bgzf.write_text(str(tmp_path / 't'), '@r\xe9\n')
    assert gzip.decompress((tmp_path / 't').read_bytes()) == b'@r\xe9\n'


# ---------------------------------------------------------------- the command line
def _parsed(monkeypatch, argv, target):
    """The keywords `kbbq <argv>` passes to `target` (module, function name), which is replaced."""
    from kbbq import main
    seen = {}
    module, name = target

    def fake(*args, **kw):
        seen.update(kw)
        return dict(k=31, min_count=2, reads=0, changed_bases=0, flagged_bases=0, changed=np.zeros(0, dtype=np.uint32), hist=None)
    monkeypatch.setattr(module, name, fake)
    from kbbq import parallel
    monkeypatch.setattr(parallel, 'init_from_env', lambda: (1, 0))
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                        # the parsers are what is under test, not the device
    for var in ('RANK', 'WORLD_SIZE'):
        monkeypatch.delenv(var, raising=False)
    main.main(argv)
    return seen


@pytest.mark.parametrize('given', [False, True])
def test_the_option_is_accepted_and_goes_down_only_when_given(monkeypatch, tmp_path, given, capsys):
    from kbbq import kmer, main, recalibrate
    from kbbq.gatk import applybqsr
    flag = ['--bgzf'] if given else []
    fq = tmp_path / 'r.fq'
    fq.write_text('@r\nACGT\n+\nFFFF\n')
    monkeypatch.setattr(main._recal, 'check_corrected', lambda *a, **k: None)
    cases = [(['recalibrate', '-f', str(fq), str(fq), '-o', 'x.gz'], (recalibrate, 'recalibrate')),
             (['recalibrate', '-c', str(fq)], (recalibrate, 'recalibrate_corrected')),
             (['correct', '-f', str(fq)], (kmer, 'main_correct')),
             (['applybqsr', '-b', 'x.sam', '-g', 'x.report'], (applybqsr, 'apply_report'))]
    for argv, target in cases:
        seen = _parsed(monkeypatch, argv + flag, target)
        assert ('bgzf' in seen) == given, argv
        if given:
            assert seen['bgzf'] is True
    assert main._bgzf_kw(type('A', (), {})()) == {}                   # a command without the option


def test_count_and_bqsr_do_not_take_the_option():
    from kbbq import main
    for argv in (['count', '-f', 'r.fq', '-o', 's', '--bgzf'], ['bqsr', '-b', 'x.sam', '-g', 'r', '--kmers', '--bgzf']):
        with pytest.raises(SystemExit):
            main.main(argv)


# ---------------------------------------------------------------- the C ABI
def test_the_symbols_are_exported_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    declared = dict(re.findall(r'^(?:int|size_t) (kbbq_bgzf_\w+)\(([^;]*)\);', header, flags=re.M))
    assert sorted(declared) == ['kbbq_bgzf_bound', 'kbbq_bgzf_deflate', 'kbbq_bgzf_deflate_dev', 'kbbq_bgzf_eof']
    assert sorted(n for n in N.PROTOTYPES if n.startswith('kbbq_bgzf_')) == sorted(declared)
    for name, params in declared.items():
        assert hasattr(lib, name)
        ret, args = N.PROTOTYPES[name]
        assert len(args) == params.count(',') + 1, name
        assert ret is (ctypes.c_size_t if name == 'kbbq_bgzf_bound' else ctypes.c_int)
    for macro, value in (('BLOCK_MAX', N.BGZF_BLOCK_MAX), ('SLOT', N.BGZF_SLOT), ('EOF_BYTES', N.BGZF_EOF_BYTES)):
        assert re.search(r'^#define KBBQ_BGZF_%s\s+%d$' % (macro, value), header, flags=re.M)
    assert lib.kbbq_abi_version() == 1


def test_the_calls_that_need_no_device():
    from kbbq import _bgzf
    from kbbq import _native as N
    lib = N.load()
    assert _bgzf.BLOCK == N.BGZF_BLOCK_MAX
    out = np.full(32, 0xAA, dtype=np.uint8)
    assert lib.kbbq_bgzf_eof(N.ptr(out)) == N.KBBQ_OK
    assert out[:28].tobytes() == EOF == _bgzf.EOF and np.all(out[28:] == 0xAA)
    assert lib.kbbq_bgzf_eof(None) == N.KBBQ_E_ARG
    assert lib.kbbq_bgzf_bound(0, 65280) == 0 and lib.kbbq_bgzf_bound(1, 65280) == 32
    assert lib.kbbq_bgzf_bound(65280, 65280) == 65311 and lib.kbbq_bgzf_bound(65281, 65280) == 65281 + 62
    assert lib.kbbq_bgzf_bound(10, 3) == 10 + 4 * 31
    assert lib.kbbq_bgzf_bound(10, 0) == 0 and lib.kbbq_bgzf_bound(10, 65281) == 0
    # refused on the arguments alone, before a context is looked at: no context exists without a device
    total = ctypes.c_size_t(7)
    for bad in (0, -1, 65281):
        assert lib.kbbq_bgzf_deflate_dev(None, None, 10, bad, None, None, None, ctypes.byref(total)) == N.KBBQ_E_ARG
        assert 'block_bytes' in N.last_error()
        assert lib.kbbq_bgzf_deflate(None, None, 10, bad, None, 0, ctypes.byref(total)) == N.KBBQ_E_ARG
        assert 'block_bytes' in N.last_error()
    assert lib.kbbq_bgzf_deflate_dev(None, None, 10, 65280, None, None, None, ctypes.byref(total)) == N.KBBQ_E_ARG
    assert lib.kbbq_bgzf_deflate(None, None, 10, 65280, None, 0, ctypes.byref(total)) == N.KBBQ_E_ARG
