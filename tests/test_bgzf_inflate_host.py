"""The host twin of the BGZF inflate kernel (csrc/kbbq_bgzf_inflate.h bi_member, through kbbq_inflate_bgzf_host) against zlib, the
block table (kbbq_inflate_index) and what the new entry points refuse without a device.  No GPU.

A valid member must come back byte for byte as zlib.decompress(payload, -15) with status 0.  A damaged member -- the fixed list
of tests/bgzf_inflate_cases.py -- must get a status, must leave the guard bytes around its output range alone, and a status of 0
may never stand beside bytes zlib does not give."""
import ctypes
import gzip
import os
import re
import struct
import zlib

import numpy as np
import pytest

import bgzf_inflate_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def twin(payload, isize, crc):
    """(status, the isize bytes of the output range) of the host twin, its output between two guard zones that must survive."""
    from kbbq import _native as N
    lib = N.load()
    src = np.frombuffer(bytes(payload), dtype=np.uint8).copy()
    buf = np.full(GUARD + isize + GUARD, 0xA5, dtype=np.uint8)
    st = lib.kbbq_inflate_bgzf_host(N.ptr(src) if src.size else None, src.size, N.ptr(buf[GUARD:]) if isize else None, isize, crc)
    assert np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + isize:] == 0xA5), 'written outside the output range'
    return st, buf[GUARD:GUARD + isize].tobytes()


@pytest.mark.parametrize('k', range(len(C.valid())), ids=[v[0] for v in C.valid()])
def test_a_valid_member_is_zlibs_bytes(k):
    name, text, payload = C.valid()[k]
    st, got = twin(payload, len(text), zlib.crc32(text))
    assert st == 0
    assert got == zlib.decompress(payload, -15) == text


def test_the_cases_are_what_they_say():
    """The members reach the paths they are named for: stored, fixed and dynamic blocks, several blocks in one member, the longest
    match at the shortest distance, the longest distance, code lengths beyond the primary table's bits."""
    import bgzf_model as M
    by = {name: (text, payload) for name, text, payload in C.valid()}
    btype = lambda p: (p[0] >> 1) & 3                                     # noqa: E731
    assert btype(by['level 0'][1]) == 0 and btype(by['Z_FIXED'][1]) == 1 and btype(by['level 6'][1]) == 2
    assert btype(by['random bytes: zlib stores them'][1]) == 0
    blocks, text = M.tokens(by['full flush: several blocks and an empty stored one'][1])
    assert len(blocks) >= 3 and text == by['level 6'][0]
    blocks, _ = M.tokens(by['65536 equal bytes: distance 1, length 258'][1])
    assert any(t[2] == (258, 1) for b in blocks for t in b['tokens'])
    blocks, _ = M.tokens(by['a repeat at distance 32768'][1])
    assert any(isinstance(t[2], tuple) and t[2][1] == 32768 for b in blocks for t in b['tokens'])
    blocks, _ = M.tokens(by['literal codes of 15 bits'][1])
    assert max(blocks[0]['ll']) > 10                                      # beyond the primary table: sub-tables
    blocks, _ = M.tokens(by['distance codes of 15 bits'][1])
    assert max(blocks[0]['d']) == 15 and len(blocks[0]['tokens']) == 256 + 16


@pytest.mark.parametrize('k', range(len(C.damaged())), ids=[d[0] for d in C.damaged()])
def test_a_damaged_member_gets_a_status(k):
    name, payload, isize, crc = C.damaged()[k]
    assert C.zlib_says(payload, isize, crc) is None, 'the case is not damaged'
    st, _ = twin(payload, isize, crc)
    assert st != 0


def test_the_statuses_name_the_damage():
    from kbbq import _native as N
    want = {'truncated in the block header': N.INFLATE_INPUT, 'truncated in the code lengths': N.INFLATE_INPUT,
            'truncated in the body': N.INFLATE_INPUT, 'a flipped CRC bit': N.INFLATE_CRC, 'a flipped ISIZE bit': N.INFLATE_ISIZE,
            'an ISIZE smaller than the output': N.INFLATE_OUTPUT, 'a distance before the start': N.INFLATE_DISTANCE,
            'literal/length symbol 286': N.INFLATE_SYMBOL, 'literal/length symbol 287': N.INFLATE_SYMBOL,
            'distance symbol 30': N.INFLATE_SYMBOL, 'distance symbol 31': N.INFLATE_SYMBOL, 'an over-subscribed code': N.INFLATE_CODE,
            'an incomplete code': N.INFLATE_CODE, 'block type 3': N.INFLATE_BTYPE, 'stored LEN / NLEN': N.INFLATE_STORED}
    for name, payload, isize, crc in C.damaged():
        if name in want:
            assert twin(payload, isize, crc)[0] == want[name], name
    # bytes behind the last deflate block: zlib and the readers' host route accept them, the twin leaves the member to the host
    name, text, payload = C.valid()[2]
    assert twin(payload + b'\0', len(text), zlib.crc32(text))[0] == N.INFLATE_TRAILING
    assert twin(payload, 65537, 0)[0] == N.INFLATE_RANGE and twin(b'\0' * 65537, 4, 0)[0] == N.INFLATE_RANGE


def test_every_single_bit_flip_of_a_small_member():
    """All 8 * len flips of a short dynamic member and of a fixed one: status 0 only beside zlib's bytes."""
    for text, payload in ((C.fastq_like(400), C.raw(C.fastq_like(400), 9)), (b'abcabcabcabc-abcabc', C.raw(b'abcabcabcabc-abcabc', 6, zlib.Z_FIXED))):
        crc, seen = zlib.crc32(text), set()
        for bit in range(8 * len(payload)):
            p = bytearray(payload)
            p[bit >> 3] ^= 1 << (bit & 7)
            st, got = twin(bytes(p), len(text), crc)
            seen.add(st)
            if st == 0:
                assert C.zlib_says(bytes(p), len(text), crc) == got
        assert len(seen - {0}) >= 4                                       # the flips reach several of the refusals


# ---------------------------------------------------------------- the block table
def test_the_index_is_headers_and_trailers_alone():
    from kbbq import _native as N
    lib = N.load()
    members = [(text, payload) for _, text, payload in C.valid()[:6]] + [(b'', C.EOF[18:-8])]
    stream = b''.join(C.frame(p, t) for t, p in members)
    src = np.frombuffer(stream, dtype=np.uint8)
    nb, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.kbbq_inflate_index(N.ptr(src), src.size, None, 0, ctypes.byref(nb), ctypes.byref(total)) == N.KBBQ_OK
    assert nb.value == len(members) and total.value == sum(len(t) for t, _ in members)
    blocks = (N.BgzfBlock * nb.value)()
    assert lib.kbbq_inflate_index(N.ptr(src), src.size, blocks, nb.value, ctypes.byref(nb), ctypes.byref(total)) == N.KBBQ_OK
    at = dst = 0
    for b, (t, p) in zip(blocks, members):
        assert (b.src, b.csize, b.dst, b.isize, b.crc) == (at + 18, len(p), dst, len(t), zlib.crc32(t))
        assert stream[b.src:b.src + b.csize] == p
        at += 18 + len(p) + 8
        dst += len(t)
    assert lib.kbbq_inflate_index(N.ptr(src), src.size, blocks, nb.value - 1, ctypes.byref(nb), ctypes.byref(total)) == N.KBBQ_E_ARG
    # a garbled payload does not change the table: nothing is inflated
    bad = bytearray(stream)
    bad[30] ^= 0xff
    bsrc = np.frombuffer(bytes(bad), dtype=np.uint8)
    assert lib.kbbq_inflate_index(N.ptr(bsrc), bsrc.size, None, 0, ctypes.byref(nb), ctypes.byref(total)) == N.KBBQ_OK
    assert nb.value == len(members)
    # not BGZF: plain gzip, a member cut short, bytes behind the last member, an ISIZE above 64 KiB, nothing at all is an empty table
    extra = C.frame(members[0][1], members[0][0])
    for other in (gzip.compress(b'hello'), stream[:-1], stream + b'\0', stream + extra[:-4] + struct.pack('<I', 65537)):
        osrc = np.frombuffer(other, dtype=np.uint8)
        assert lib.kbbq_inflate_index(N.ptr(osrc), osrc.size, None, 0, ctypes.byref(nb), ctypes.byref(total)) == N.INFLATE_NOT_BGZF
        assert nb.value == 0 and total.value == 0
    assert lib.kbbq_inflate_index(None, 0, None, 0, ctypes.byref(nb), ctypes.byref(total)) == N.KBBQ_OK and nb.value == 0
    assert lib.kbbq_inflate_index(N.ptr(src), src.size, None, 0, None, ctypes.byref(total)) == N.KBBQ_E_ARG


# ---------------------------------------------------------------- the C ABI
def test_the_symbols_are_exported_declared_and_prototyped():
    from kbbq import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    declared = dict(re.findall(r'^int (kbbq_inflate_\w+)\(([^;]*)\);', header, flags=re.M))
    assert sorted(declared) == ['kbbq_inflate_bgzf', 'kbbq_inflate_bgzf_dev', 'kbbq_inflate_bgzf_host', 'kbbq_inflate_index',
                                'kbbq_inflate_stats_get', 'kbbq_inflate_use_ctx']
    assert sorted(n for n in N.PROTOTYPES if n.startswith('kbbq_inflate_')) == sorted(declared)
    for name, params in declared.items():
        assert hasattr(lib, name)
        ret, args = N.PROTOTYPES[name]
        assert len(args) == params.count(',') + 1 and ret is ctypes.c_int, name
    assert ctypes.sizeof(N.BgzfBlock) == 32 and ctypes.sizeof(N.InflateStats) == 32
    names = re.search(r'enum \{\s*(KBBQ_INFLATE_OK[^}]*)\}', header).group(1)
    names = [x.strip().split(' ')[0] for x in names.split(',')]
    assert [getattr(N, x[5:]) for x in names] == list(range(len(names))) and len(names) == 13


def test_the_calls_refuse_their_arguments_before_any_device_is_looked_at():
    from kbbq import _native as N
    lib = N.load()
    got, st = ctypes.c_size_t(7), N.InflateStats()
    assert lib.kbbq_inflate_bgzf(None, None, 10, None, 0, ctypes.byref(got), ctypes.byref(st)) == N.KBBQ_E_ARG
    assert 'kbbq_inflate_bgzf' in N.last_error()
    assert lib.kbbq_inflate_bgzf_dev(None, None, 0, None, 1, None, 0, None) == N.KBBQ_E_ARG
    assert 'kbbq_inflate_bgzf_dev' in N.last_error()
    assert lib.kbbq_inflate_stats_get(None) == N.KBBQ_E_ARG
    assert lib.kbbq_inflate_stats_get(ctypes.byref(st)) == N.KBBQ_OK
    assert lib.kbbq_inflate_use_ctx(None) == N.KBBQ_OK


# ---------------------------------------------------------------- the readers without a context
def test_the_readers_stay_on_the_host_without_a_context(tmp_path, monkeypatch):
    """KBBQ_GPU_INFLATE=1 with a threshold of 0 and no registered context: the reader inflates on the host as it always has, and
    the device-block counter stays where it was."""
    from kbbq import _bgzf
    from kbbq import _native as N
    lib = N.load()
    text = C.fastq_like(150000)
    path = tmp_path / 'x.txt.gz'
    path.write_bytes(b''.join(C.frame(C.raw(text[i:i + 65280]), text[i:i + 65280]) for i in range(0, len(text), 65280)) + C.EOF)
    before = _bgzf.inflate_stats()
    monkeypatch.setenv('KBBQ_GPU_INFLATE', '1')
    monkeypatch.setenv('KBBQ_GPU_INFLATE_MIN_BYTES', '0')
    assert lib.kbbq_inflate_use_ctx(None) == N.KBBQ_OK
    handle, data, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(0)
    N.check(lib.kbbq_text_open(str(path).encode(), ctypes.byref(handle), ctypes.byref(data), ctypes.byref(n)))
    try:
        assert ctypes.string_at(data, n.value) == text
    finally:
        lib.kbbq_text_close(handle)
    assert _bgzf.inflate_stats() == before


def test_wants_device(tmp_path, monkeypatch):
    from kbbq import _bgzf
    gz, plain = tmp_path / 'a.gz', tmp_path / 'a.txt'
    gz.write_bytes(C.frame(C.raw(b'x' * 5000), b'x' * 5000) + C.EOF)
    plain.write_bytes(b'x' * 5000)
    monkeypatch.delenv('KBBQ_GPU_INFLATE', raising=False)
    monkeypatch.setenv('KBBQ_GPU_INFLATE_MIN_BYTES', '0')
    assert not _bgzf.wants_device(str(gz))                                # off unless asked for
    monkeypatch.setenv('KBBQ_GPU_INFLATE', '1')
    assert _bgzf.wants_device(str(plain), str(gz)) and _bgzf.wants_device(None, str(gz))
    assert not _bgzf.wants_device(str(plain)) and not _bgzf.wants_device(str(tmp_path / 'missing.gz'))
    monkeypatch.delenv('KBBQ_GPU_INFLATE_MIN_BYTES')
    assert not _bgzf.wants_device(str(gz))                                # below the default threshold of 1 MiB
    monkeypatch.setenv('KBBQ_GPU_INFLATE', '0')
    monkeypatch.setenv('KBBQ_GPU_INFLATE_MIN_BYTES', '0')
    assert not _bgzf.wants_device(str(gz))
