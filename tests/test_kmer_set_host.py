"""K-mer sets without a GPU: the format's model on a hand-worked case, the header's round trip and every refusal that needs no
device (raised with no library load), `--kmers-from`'s argparse errors on the five commands and `kbbq count`'s refusals (before a
process group could be joined), what main forwards to the drivers, the keyword's way down only when it is given, the place of
` kmers_from=1 loaded_kmers=N` at the end of each stderr line, and the new symbols in the header, the library and the
prototypes."""
import os
import re
import struct

import numpy as np
import pytest

import kmer_set_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _never(*a, **kw):
    raise AssertionError('a device call, a library load or a process group')


# ---------------------------------------------------------------- the model, by hand
# k = 8, two copies of ACGTTGCAAG: windows ACGTTGCA, CGTTGCAA, GTTGCAAG (A C G T = 0 1 2 3, first base in the high bits)
#   ACGTTGCA = 0 1 2 3 3 2 1 0 -> 4096 + 2048 + 768 + 192 + 32 + 4          =  7140; reverse complement TGCAACGT = 58395
#   CGTTGCAA = 1 2 3 3 2 1 0 0 -> 16384 + 8192 + 3072 + 768 + 128 + 16      = 28560; reverse complement TTGCAACG = 63750
#   GTTGCAAG = 2 3 3 2 1 0 0 2 -> 32768 + 12288 + 3072 + 512 + 64 + 2       = 48706; reverse complement CTTGCAAC = 32321 (canonical)
HAND_KEYS, HAND_COUNTS = (7140, 28560, 32321), (2, 2, 2)


def _hand_bytes(keep=2, n=3):
    hist = [0] * 257
    hist[2] = 3
    keys, counts = HAND_KEYS[:n], HAND_COUNTS[:n]
    out = b'KBBQKMER'
    out += struct.pack('<I', 1) + struct.pack('<I', 8) + struct.pack('<I', keep) + struct.pack('<I', 0)
    out += struct.pack('<Q', n)                     # n
    out += struct.pack('<Q', 2)                     # reads
    out += struct.pack('<Q', 6)                     # windows: three of each copy
    out += struct.pack('<Q', sum(keys))             # key_sum
    out += struct.pack('<Q', sum(counts))           # count_sum
    out += struct.pack('<257Q', *hist)
    out += struct.pack('<%dQ' % n, *keys) + struct.pack('<%dI' % n, *counts)
    return out


def test_the_models_bytes_of_a_hand_worked_case():
    records = [(b'ACGTTGCAAG', None)] * 2
    keys, counts = SM.count(records, 8)
    assert tuple(keys.tolist()) == HAND_KEYS and tuple(counts.tolist()) == HAND_COUNTS
    data = SM.set_bytes(records, 8, 2)
    assert data == _hand_bytes() and len(data) == 2120 + 12 * 3 == 2156
    assert sum(HAND_KEYS) == 68021
    f = SM.parse(data)
    assert (f['magic'], f['version'], f['k'], f['keep'], f['min_qual'], f['n'], f['reads'], f['windows'], f['key_sum'], f['count_sum']) \
        == (b'KBBQKMER', 1, 8, 2, 0, 3, 2, 6, 68021, 6)
    assert f['hist'][2] == 3 and int(f['hist'].sum()) == 3
    # keep = 1 writes the same pairs and histogram; keep = 3 an empty set whose histogram is all zero
    assert SM.set_bytes(records, 8, 1) == _hand_bytes(keep=1)
    empty = SM.parse(SM.set_bytes(records, 8, 3))
    assert empty['n'] == 0 and int(empty['hist'].sum()) == 0 and empty['windows'] == 6 and (empty['key_sum'], empty['count_sum']) == (0, 0)
    # a gate that takes the last base away takes the last window: ACGTTGCA and CGTTGCAA stay
    gated = SM.parse(SM.set_bytes([(b'ACGTTGCAAG', b'IIIIIIIII#')] * 2, 8, 2, Q=20))
    assert tuple(gated['keys'].tolist()) == HAND_KEYS[:2] and gated['min_qual'] == 20 and gated['windows'] == 4
    # the split of the reads over records of a multiset does not matter, their order neither
    a, b = (b'ACGTTGCAAGTTTTTTTT', None), (b'GGGGGGGGGACGTTGCA', None)
    assert SM.set_bytes([a, b, a], 8, 1)[32:] == SM.set_bytes([b, a, a], 8, 1)[32:]


def test_the_models_pair_check():
    f = SM.parse(_hand_bytes())
    ok = (f['keys'], f['counts'], 8, 2, f['key_sum'], f['count_sum'])
    assert SM.check_pairs(*ok) is None
    keys, counts = f['keys'].copy(), f['counts'].copy()
    swapped = keys.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert SM.check_pairs(swapped, counts, 8, 2, f['key_sum'], f['count_sum']) == (1, SM.ORDER)
    twice = keys.copy()
    twice[2] = twice[1]
    assert SM.check_pairs(twice, counts, 8, 2, 0, 0) == (2, SM.ORDER)
    far = keys.copy()
    far[2] = 4 ** 8
    assert SM.check_pairs(far, counts, 8, 2, 0, 0) == (2, SM.RANGE)
    other = keys.copy()
    other[2] = 48706                                  # GTTGCAAG itself, above its reverse complement
    assert SM.check_pairs(other, counts, 8, 2, 0, 0) == (2, SM.CANONICAL)
    low = counts.copy()
    low[1] = 1
    assert SM.check_pairs(keys, low, 8, 2, 0, 0) == (1, SM.COUNT)
    assert SM.check_pairs(keys, counts, 8, 2, f['key_sum'] + 1, f['count_sum']) == 'checksum'
    assert SM.check_pairs(keys, counts, 8, 2, f['key_sum'], f['count_sum'] - 1) == 'checksum'
    # k = 32: a key with bit 63 set is in range, and ascending means ascending as unsigned
    g16c16 = int('10' * 16 + '01' * 16, 2)
    assert g16c16 >> 63 == 1
    assert SM.check_pairs(np.array([0, g16c16], dtype=np.uint64), [2, 2], 32, 2, g16c16, 4) is None
    assert SM.check_pairs(np.array([g16c16, 0], dtype=np.uint64), [2, 2], 32, 2, g16c16, 4) == (1, SM.ORDER)


# ---------------------------------------------------------------- the header
def test_header_round_trip_and_the_writer(tmp_path):
    from kbbq import kmerset
    assert kmerset.HEADER_BYTES == 2120 and kmerset.MAGIC == b'KBBQKMER' and kmerset.VERSION == 1
    hist = np.zeros(257, dtype=np.int64)
    hist[2], hist[256] = 3, 1
    g16c16 = int('10' * 16 + '01' * 16, 2)
    head = kmerset.pack_header(32, 2, 20, 4, 7, 99, (1 << 64) + 5, 6, hist)
    assert len(head) == 2120
    s = kmerset.unpack_header(head, 'x.set', 2120 + 48)
    assert (s.path, s.k, s.keep, s.min_qual, s.n, s.reads, s.windows, s.key_sum, s.count_sum) == ('x.set', 32, 2, 20, 4, 7, 99, 5, 6)
    assert np.array_equal(s.hist, hist) and s.hist.dtype == np.int64
    assert (s.keys_offset, s.counts_offset, s.nbytes) == (2120, 2120 + 32, 2120 + 48)
    # write_set -> the model's bytes -> open_set
    path = str(tmp_path / 'a.set')
    keys = np.array([0, 5, 7, g16c16], dtype=np.uint64)
    counts = np.array([2, 2, 2, 300], dtype=np.uint32)
    ksum = int(keys.sum(dtype=np.uint64))
    kmerset.write_set(path, 32, 2, 0, 7, 99, hist, ksum, 306,
                      lambda what: iter((keys[:3], keys[3:]) if what == 'keys' else (counts[:1], counts[1:])), 4)
    data = open(path, 'rb').read()
    assert data == SM.file_bytes(32, 2, 0, 7, 99, hist, keys, counts)
    f = kmerset.open_set(path)
    assert (f.k, f.keep, f.n, f.key_sum, f.count_sum) == (32, 2, 4, ksum, 306)
    # an existing file is never overwritten, and a failed write leaves nothing behind
    with pytest.raises(FileExistsError):
        kmerset.write_set(path, 32, 2, 0, 7, 99, hist, ksum, 306, lambda what: iter(()), 4)
    assert open(path, 'rb').read() == data
    with pytest.raises(ValueError, match='3 keys for n = 4'):
        kmerset.write_set(str(tmp_path / 'b.set'), 32, 2, 0, 7, 99, hist, ksum, 306, lambda what: iter((keys[:3],)), 4)
    assert not os.path.exists(str(tmp_path / 'b.set'))
    # the threshold of a set: solid_threshold up to keep = 2, the first valley at or above a larger keep
    from kbbq import kmer
    h = np.zeros(257, dtype=np.int64)
    h[2:8] = [50, 20, 5, 9, 30, 10]
    assert kmerset.set_threshold(h, 1) == kmerset.set_threshold(h, 2) == kmer.solid_threshold(h) == 4
    h3 = h.copy()
    h3[:5] = 0
    assert kmer.solid_threshold(h3) == 2 and kmerset.set_threshold(h3, 5) == 5 and kmerset.set_threshold(h, 5) == 5
    with pytest.raises(ValueError, match=r'no valley in 2\.\.255: give min_count'):
        kmerset.set_threshold(np.arange(257, 0, -1), 2)
    assert kmerset.slab_pairs() == (96 << 20) // 12


def test_every_header_level_refusal_needs_no_library(monkeypatch, tmp_path):
    from kbbq import _native, kmer, kmerset
    monkeypatch.setattr(_native, 'load', _never)
    monkeypatch.setattr(kmer, '_ctx', _never)
    good = _hand_bytes()
    path = str(tmp_path / 'x.set')

    def refused(data, message, call=None):
        with open(path, 'wb') as fh:
            fh.write(data)
        for f in (kmerset.open_set, lambda p: kmer.load_set(p), lambda p: kmer.load_set(p, min_count=3, slots=1024)) \
                if call is None else (call,):
            with pytest.raises(ValueError, match=message) as exc:
                f(path)
            assert str(exc.value).startswith('k-mer set %s: ' % path) or call is not None

    def edit(offset, fmt, value):
        return good[:offset] + struct.pack(fmt, value) + good[offset + struct.calcsize(fmt):]
    refused(b'KBBQKMEX' + good[8:], 'not a k-mer set')
    refused(b'@r1\nACGT\n+\nIIII\n' * 200, 'not a k-mer set')
    refused(good[:100], r'100 bytes are no header \(2120 bytes\)')
    refused(b'', '0 bytes are no header')
    refused(edit(8, '<I', 2), 'version 2, this build reads version 1')
    refused(edit(12, '<I', 7), r'k must be in 8\.\.32, got 7')
    refused(edit(12, '<I', 33), r'k must be in 8\.\.32, got 33')
    refused(edit(16, '<I', 0), 'keep must be >= 1, got 0')
    refused(good + b'\0', r'2157 bytes, but n = 3 pairs make 2156')
    refused(good[:-4], r'2152 bytes, but n = 3 pairs make 2156')
    refused(edit(24, '<Q', 4) + b'\0' * 12, r'n = 4 pairs but sum\(hist\[2:\]\) = 3')
    refused(edit(64 + 8 * 3, '<Q', 1), r'n = 3 pairs but sum\(hist\[2:\]\) = 4')
    refused(edit(64 + 8 * 1, '<Q', 5), r'hist\[1\] = 5 below keep = 2 must be 0')
    # ... and what load_set refuses on the header and its arguments alone
    with open(path, 'wb') as fh:
        fh.write(good)
    assert kmerset.open_set(path).n == 3 and kmer.set_k(path) == 8 and kmer.set_k(path, 8) == 8
    for call in (lambda: kmer.load_set(path, k=31), lambda: kmer.set_k(path, 31)):
        with pytest.raises(ValueError, match=r'k = 31 was asked for, but the k-mer set .*x\.set was counted with k = 8'):
            call()
    with pytest.raises(ValueError, match=r'min_count = 1 is below keep = 2 of the k-mer set'):
        kmer.load_set(path, min_count=1)
    hist = np.zeros(257, dtype=np.int64)                 # strictly falling: no valley
    hist[2:] = np.arange(255, 0, -1)
    n = int(hist.sum())
    with open(path, 'wb') as fh:
        fh.write(SM.file_bytes(8, 2, 0, 2, 6, hist, np.arange(n), np.full(n, 2)))
    with pytest.raises(ValueError, match='no valley in 2..255: give min_count'):
        kmer.load_set(path)
    with pytest.raises(FileNotFoundError):
        kmer.load_set(str(tmp_path / 'absent.set'))


# ---------------------------------------------------------------- kmers_from refuses counting options, everywhere, with no device
def test_python_refuses_counting_options_before_any_device_call(monkeypatch, tmp_path):
    from kbbq import _native, benchmark, kmer, recalibrate
    from kbbq.gatk import bqsr
    monkeypatch.setattr(_native, 'load', _never)
    monkeypatch.setattr(kmer, '_ctx', _never)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    assert kmer.check_kmers_from(None, prefilter=True, partitions=3) is None          # nothing to refuse without a set
    assert kmer.check_kmers_from('s.set') == 's.set' and kmer.check_kmers_from(tmp_path / 's.set') == str(tmp_path / 's.set')
    assert kmer._kmers_from_kw(None) == {} and kmer._kmers_from_kw('s') == dict(kmers_from='s')
    assert kmer.kmers_from_field({}) == '' and kmer.kmers_from_field(dict(kmers_from=None, loaded_kmers=3)) == ''
    assert kmer.kmers_from_field(dict(kmers_from='s.set', loaded_kmers=3)) == ' kmers_from=1 loaded_kmers=3'
    seq, meta = np.full((2, 48), ord('A'), dtype=np.uint8), np.array([40, 40], dtype=np.uint32)
    options = (dict(prefilter=True), dict(filter_bits=8), dict(partitions=2), dict(partitions='auto'), dict(kmer_min_qual=20))
    for opt in options:
        name = next(iter(opt))
        calls = [lambda: kmer.correct_reads(seq, meta, kmers_from='s.set', **opt),
                 lambda: kmer.correct_fastq('x.fq', 'y.fq', kmers_from='s.set', **opt),
                 lambda: kmer.main_correct('x.fq', kmers_from='s.set', **opt),
                 lambda: recalibrate.recalibrate_corrected('x.fq', kmers_from='s.set', **opt),
                 lambda: recalibrate.check_bam_kmers('x.sam', kmers_from='s.set', **opt),
                 lambda: recalibrate.recalibrate_bam('x.sam', kmers=dict(kmers_from='s.set', **opt)),
                 lambda: bqsr.bam_to_kmer_covariates('x.sam', kmers_from='s.set', **opt),
                 lambda: benchmark.benchmark_kmers('x.sam', {}, {}, kmers_from='s.set', **opt)]
        if name == 'kmer_min_qual':
            calls.append(lambda: kmer.correct_fastq_ranks('x.fq', 'y.fq', kmers_from='s.set', **opt))
        for call in calls:
            with pytest.raises(ValueError, match='%s: not with kmers_from: these are counting options' % name):
                call()
    for call in (lambda: kmer.correct_fastq('x.fq', 'y.fq', kmers_from='s.set', local_slots=64),
                 lambda: kmer.main_correct('x.fq', kmers_from='s.set', local_slots=64),
                 lambda: kmer.correct_fastq_ranks('x.fq', 'y.fq', kmers_from='s.set', local_slots=64)):
        with pytest.raises(ValueError, match='local_slots: not with kmers_from'):
            call()
    with pytest.raises(ValueError, match='prefilter, partitions, kmer_min_qual: not with kmers_from'):
        kmer.check_kmers_from('s.set', True, 4, 3, 20)
    # a set of another k than the one asked for, or one that is no set, is refused on its header: still no device
    path = str(tmp_path / 'k8.set')
    with open(path, 'wb') as fh:
        fh.write(_hand_bytes())
    for call in (lambda: kmer.correct_reads(seq, meta, k=31, kmers_from=path),
                 lambda: recalibrate.recalibrate_corrected('x.fq', k=31, kmers_from=path),
                 lambda: benchmark.benchmark_kmers('x.sam', {}, {}, k=31, kmers_from=path)):
        with pytest.raises(ValueError, match='k = 31 was asked for, but the k-mer set .* was counted with k = 8'):
            call()


# ---------------------------------------------------------------- command line
def _no_ranks(monkeypatch):
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')            # the commands then leave the memory back end alone


COMMANDS = (['correct', '-f', 'x.fq'], ['recalibrate', '-c', 'x.fq'], ['recalibrate', '-b', 'x.sam', '--kmers'],
            ['bqsr', '-b', 'x', '--kmers', '-g', 'r'], ['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '--kmers'])
_ids = lambda c: '-'.join(c[:2] + c[3:4])


def _nothing_runs(monkeypatch):
    from kbbq import benchmark as bm, kmer, kmerset, main, parallel, recalibrate as recal
    from kbbq.gatk import bqsr
    monkeypatch.setattr(parallel, 'init_from_env', _never)              # before the ranks join
    monkeypatch.setattr(recal, 'recalibrate', lambda **kw: pytest.fail('ran'))
    monkeypatch.setattr(recal, 'recalibrate_corrected', lambda *a, **kw: pytest.fail('ran'))
    monkeypatch.setattr(recal, 'recalibrate_bam', lambda *a, **kw: pytest.fail('ran'))
    monkeypatch.setattr(bm, 'benchmark', lambda **kw: pytest.fail('ran'))
    monkeypatch.setattr(bqsr, 'bam_to_report', lambda *a: pytest.fail('ran'))
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', lambda *a, **kw: pytest.fail('ran'))
    monkeypatch.setattr(kmer, 'main_correct', lambda *a, **kw: pytest.fail('ran'))
    monkeypatch.setattr(kmerset, 'count', lambda *a, **kw: pytest.fail('ran'))
    return main


@pytest.mark.parametrize('command', COMMANDS, ids=_ids)
@pytest.mark.parametrize('option', (['--prefilter'], ['--filter-bits', '8'], ['--partitions', '2'], ['--partitions', 'auto'],
                                    ['--kmer-min-qual', '20'], ['--prefilter', '--partitions', '3']), ids=lambda o: o[0][2:] + o[-1])
def test_counting_options_with_kmers_from_are_argparse_errors(monkeypatch, capsys, command, option):
    main = _nothing_runs(monkeypatch)
    _no_ranks(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(command + ['--kmers-from', 's.set'] + option)
    assert exc.value.code == 2
    err = capsys.readouterr().err
    assert '%s: not with --kmers-from' % ', '.join(o for o in option if o.startswith('--')) in err


def test_local_slots_too_and_a_launched_rank_gets_the_same_error(monkeypatch, capsys):
    main = _nothing_runs(monkeypatch)
    _no_ranks(monkeypatch)
    for env in ({}, dict(RANK='1', WORLD_SIZE='2')):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(SystemExit) as exc:
            main.main(['correct', '-f', 'x.fq', '--kmers-from', 's.set', '--local-slots', '64'])
        assert exc.value.code == 2 and '--local-slots: not with --kmers-from' in capsys.readouterr().err


@pytest.mark.parametrize('argv, message', (
    (['recalibrate', '-f', 'a.fq', 'b.fq', '--kmers-from', 's'], '--kmers-from: only with -c/--correct or with -b --kmers'),
    (['recalibrate', '-b', 'a.bam', '--kmers-from', 's'], '--kmers-from: only with -c/--correct or with -b --kmers'),
    (['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r', '--kmers-from', 's'], '--kmers-from: only with --kmers'),
    (['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '--kmers-from', 's'], '--kmers-from: only with --kmers'),
))
def test_kmers_from_only_with_the_k_mer_form(monkeypatch, capsys, argv, message):
    main = _nothing_runs(monkeypatch)
    _no_ranks(monkeypatch)
    with pytest.raises(SystemExit) as exc:
        main.main(argv)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


class _Report:
    def write(self, path):
        pass


def test_the_option_reaches_the_commands_only_when_given_and_the_field_comes_last(monkeypatch, capsys):
    from kbbq import aln, benchmark as bm, kmer, main, recalibrate as recal
    from kbbq.gatk import bqsr
    _no_ranks(monkeypatch)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    seen = []
    given = ['--kmers-from', 's.set']
    rest = ['--passes', '2', '--min-count', '5', '--slots', '64']

    def loaded(info, kw):
        if kw.get('kmers_from') is not None:
            info.update(kmers_from=kw['kmers_from'], loaded_kmers=41, k=15 if kw['k'] is None else kw['k'])
        return info

    # correct: main.correct -> kmer.main_correct -> kmer.correct_fastq; -k is the set's unless it is given
    def correct_fastq(path, out, **kw):
        seen.append(kw)
        return loaded(dict(k=kw['k'], min_count=4, reads=9, changed=np.array([1, 2])), kw)
    monkeypatch.setattr(kmer, 'correct_fastq', correct_fastq)
    for more in ([], given, given + rest + ['--fix-n', '-k', '21']):
        main.main(['correct', '-f', 'x.fq'] + more)
    assert 'kmers_from' not in seen[0] and seen[0]['k'] == 31 and seen[0]['filter_bits'] == 4 and seen[0]['prefilter'] is False
    assert seen[1]['kmers_from'] == seen[2]['kmers_from'] == 's.set' and seen[1]['k'] is None and seen[2]['k'] == 21
    assert (seen[2]['min_count'], seen[2]['slots'], seen[2]['passes']) == (5, 64, 2)
    assert capsys.readouterr().err.splitlines() == [
        'kbbq correct: k=31 min_count=4 reads=9 changed_bases=3',
        'kbbq correct: k=15 min_count=4 reads=9 changed_bases=3 kmers_from=1 loaded_kmers=41',
        'kbbq correct: k=21 min_count=4 reads=9 changed_bases=3 fix_n=1 passes=2 kmers_from=1 loaded_kmers=41']

    # recalibrate -c
    del seen[:]
    monkeypatch.setattr(recal, 'check_corrected', lambda *a, **kw: seen.append(('checked', a[2])))
    monkeypatch.setattr(recal, 'recalibrate_corrected', lambda path, **kw: seen.append(kw) or loaded(
        dict(k=kw['k'], min_count=3, reads=5, changed_bases=7, skipped_bases=2), kw))
    for more in ([], given, given + rest + ['--skip-unresolved', '--fix-n', '-k', '21']):
        main.main(['recalibrate', '-c', 'x.fq'] + more)
    assert [x[1] for x in seen[0::2]] == [31, 31, 21]                               # check_corrected gets a k to check
    runs = seen[1::2]
    assert 'kmers_from' not in runs[0] and runs[0]['k'] == 31
    assert runs[1]['kmers_from'] == runs[2]['kmers_from'] == 's.set' and runs[1]['k'] is None and runs[2]['k'] == 21
    assert [x for x in capsys.readouterr().err.splitlines() if x.startswith('kbbq ')] == [
        'kbbq recalibrate: k=31 min_count=3 reads=5 changed_bases=7',
        'kbbq recalibrate: k=15 min_count=3 reads=5 changed_bases=7 kmers_from=1 loaded_kmers=41',
        'kbbq recalibrate: k=21 min_count=3 reads=5 changed_bases=7 skipped_bases=2 fix_n=1 passes=2 kmers_from=1 loaded_kmers=41']

    # bqsr --kmers
    del seen[:]

    def kmers(bam, **kw):
        seen.append(kw)
        kw['info'].update(k=kw['k'], min_count=7, reads=5, flagged_bases=11, skipped_bases=17, excluded_reads=1)
        loaded(kw['info'], kw)
        return _Report()
    monkeypatch.setattr(aln, 'AlignmentFile', lambda p: 'opened:' + p)
    monkeypatch.setattr(bqsr, 'bam_to_report_kmers', kmers)
    for more in ([], given, given + rest + ['--skip-unresolved', '--mixed-lengths', '-F', '0x400']):
        main.main(['bqsr', '-b', 'x.bam', '--kmers', '-g', 'r.grp'] + more)
    assert 'kmers_from' not in seen[0] and seen[0]['k'] == 31
    assert seen[1]['kmers_from'] == seen[2]['kmers_from'] == 's.set' and seen[1]['k'] is None
    assert capsys.readouterr().err.splitlines() == [
        'kbbq bqsr: k=31 min_count=7 reads=5 flagged_bases=11',
        'kbbq bqsr: k=15 min_count=7 reads=5 flagged_bases=11 kmers_from=1 loaded_kmers=41',
        'kbbq bqsr: k=15 min_count=7 reads=5 excluded_reads=1 flagged_bases=11 skipped_bases=17 passes=2 kmers_from=1 loaded_kmers=41']

    # recalibrate -b --kmers
    del seen[:]
    checked = []
    monkeypatch.setattr(recal, 'check_bam_kmers', lambda *a, **kw: checked.append((a[3], kw)))
    monkeypatch.setattr(recal, 'check_bam_records', lambda *a, **kw: checked.append(a[2]))
    monkeypatch.setattr(recal, 'recalibrate_bam', lambda bam, **kw: seen.append(kw['kmers']) or loaded(
        dict(k=kw['kmers']['k'], min_count=7, reads=5, flagged_bases=11), kw['kmers']))
    for more in ([], given):
        main.main(['recalibrate', '-b', 'x.sam', '--kmers'] + more)
    assert 'kmers_from' not in seen[0] and seen[0]['k'] == 31 and seen[1]['kmers_from'] == 's.set' and seen[1]['k'] is None
    assert checked[0] == (31, {}) and checked[1] == 31 and checked[2] == (None, dict(kmers_from='s.set')) and checked[3] == 31
    assert [x for x in capsys.readouterr().err.splitlines() if x.startswith('kbbq ')] == [
        'kbbq recalibrate: k=31 min_count=7 reads=5 flagged_bases=11',
        'kbbq recalibrate: k=15 min_count=7 reads=5 flagged_bases=11 kmers_from=1 loaded_kmers=41']

    # benchmark --kmers
    del seen[:]
    monkeypatch.setattr(bm, 'benchmark', lambda **kw: seen.append(kw))
    for more in ([], given, given + ['-k', '21']):
        main.main(['benchmark', '-b', 'x.sam', '-r', 'x.fa', '-v', 'x.vcf', '--kmers'] + more)
    assert 'kmers_from' not in seen[0]['kmers'] and seen[1]['kmers'] == dict(seen[0]['kmers'], kmers_from='s.set', k=None)
    assert seen[2]['kmers']['k'] == 21
    info = dict(k=31, min_count=4, reads=9, bases=100, errors=10, flagged=8, flagged_errors=8, unresolved=5, unresolved_errors=1,
                prefilter=False, admitted=None, slots=64)
    line = bm.kmer_summary(info)
    assert bm.kmer_summary(dict(info, kmers_from=None)) == line and 'kmers_from' not in line
    assert bm.kmer_summary(dict(info, passes=3, kmers_from='s.set', loaded_kmers=41)) == line + ' passes=3 kmers_from=1 loaded_kmers=41'


def test_the_keyword_goes_down_only_when_given(monkeypatch):
    from kbbq import kmer
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    seen = {}

    def fake(path, out, **kw):
        seen.update(kw=kw)
        return dict(k=15, min_count=4, reads=9, changed=np.array([1]), **({'kmers_from': kw['kmers_from'], 'loaded_kmers': 2}
                                                                         if 'kmers_from' in kw else {}))
    monkeypatch.setattr(kmer, 'correct_fastq', fake)
    kmer.main_correct('x.fq')
    assert 'kmers_from' not in seen['kw']
    kmer.main_correct('x.fq', k=None, kmers_from='s.set')
    assert seen['kw']['kmers_from'] == 's.set' and seen['kw']['k'] is None


# ---------------------------------------------------------------- kbbq count
def test_counts_refusals_come_before_any_device_call_and_any_group(monkeypatch, tmp_path):
    from kbbq import _native, kmer, kmerset, parallel
    monkeypatch.setattr(_native, 'load', _never)
    monkeypatch.setattr(kmer, '_ctx', _never)
    monkeypatch.setattr(parallel, 'init_from_env', _never)
    for name in ('all_gather_object', 'barrier', 'raise_first_error', 'sum_over_ranks', 'broadcast_object'):
        monkeypatch.setattr(parallel, name, _never)
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    out = str(tmp_path / 'new.set')
    there = tmp_path / 'there.set'
    there.write_bytes(b'kept')

    def refused(message, *a, **kw):
        for f in (kmerset.check_count, kmerset.count, kmerset.main_count):
            with pytest.raises(ValueError, match=message):
                f(*a, **kw)
    refused('kbbq count needs at least one input', (), (), out)
    refused('kbbq count needs -o SET', ['x.fq'], (), None)
    refused('the k-mer set .*there.set exists: kbbq count does not overwrite', ['x.fq'], (), str(there))
    refused(r'k must be in 8\.\.32, got 7', ['x.fq'], (), out, k=7)
    refused(r'k must be in 8\.\.32, got 33', (), ['x.sam'], out, k=33)
    refused('keep must be an integer >= 1, got 0', ['x.fq'], (), out, keep=0)
    refused('keep must be an integer >= 1, got 2.5', ['x.fq'], (), out, keep=2.5)
    refused('keep must be >= 2 with the prefilter, got 1: k-mers seen once are not counted', ['x.fq'], (), out, keep=1, prefilter=True)
    refused(r'filter_bits must be in 1\.\.64, got 65', ['x.fq'], (), out, prefilter=True, filter_bits=65)
    refused(r'-u/--use-oq: only with -b', ['x.fq'], (), out, use_oq=True)
    refused(r'-F/--exclude-flags: only with -b', ['x.fq'], (), out, exclude_flags=0x400)
    refused(r'exclude_flags must be an integer in 0\.\.0xFFFF', ['x.fq'], ['x.sam'], out, exclude_flags=1 << 16)
    refused(r"partitions must be an integer in 1\.\.64 or 'auto', got 65", ['x.fq'], (), out, partitions=65)
    refused(r'kmer_min_qual must be an integer in 1\.\.93, got 94', ['x.fq'], (), out, kmer_min_qual=94)
    assert there.read_bytes() == b'kept' and not os.path.exists(out)
    inputs, P, Q, F = kmerset.check_count(['a.fq', 'b.fq'], ['c.sam'], out, 15, 3, True, 8, 'auto', 20, True, 0x400)
    assert inputs == [('fastq', 'a.fq'), ('fastq', 'b.fq'), ('aln', 'c.sam')] and (P, Q, F) == ('auto', 20, 0x400)
    # a rank of a launcher, or of a group that exists: the first refusal, whatever else is wrong, before the group is joined
    for env in (dict(RANK='0', WORLD_SIZE='2'), dict(RANK='0', WORLD_SIZE='1', KBBQ_DIST_ALWAYS='1')):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        refused('kbbq count runs on one GPU', ['x.fq'], (), out)
        refused('kbbq count runs on one GPU', (), (), None, k=7)
        for k in env:
            monkeypatch.delenv(k)
    monkeypatch.setattr(kmer, '_ranks', lambda: (2, 1))
    refused('kbbq count runs on one GPU', ['x.fq'], (), out)


def test_what_main_forwards_to_count(monkeypatch, capsys, tmp_path):
    from kbbq import kmerset, main, parallel
    _no_ranks(monkeypatch)
    monkeypatch.setattr(parallel, 'init_from_env', _never)              # count never joins a group
    seen = []
    monkeypatch.setattr(kmerset, 'check_count', lambda *a: seen.append(('check', a)))
    monkeypatch.setattr(kmerset, 'main_count', lambda *a, **kw: seen.append(('count', a, kw)))
    main.main(['count', '-f', 'a.fq', 'b.fq', '-o', 'o.set'])
    main.main(['count', '-b', 'a.sam', '-f', 'r.fq', '-o', 'o.set', '-k', '15', '--keep', '3', '--slots', '64', '--prefilter', '--filter-bits',
               '8', '--partitions', 'auto', '--kmer-min-qual', '20', '-u', '-F', '0x400', '--histo', 'h.tsv'])
    assert seen[0] == ('check', (['a.fq', 'b.fq'], [], 'o.set', 31, 2, False, 4, 1, None, False, 0))
    assert seen[1] == ('count', (['a.fq', 'b.fq'], [], 'o.set'),
                       dict(k=31, keep=2, slots=None, prefilter=False, filter_bits=4, partitions=1, kmer_min_qual=None, use_oq=False,
                            exclude_flags=0, histo=None))
    assert seen[2] == ('check', (['r.fq'], ['a.sam'], 'o.set', 15, 3, True, 8, 'auto', 20, True, 0x400))
    assert seen[3] == ('count', (['r.fq'], ['a.sam'], 'o.set'),
                       dict(k=15, keep=3, slots=64, prefilter=True, filter_bits=8, partitions='auto', kmer_min_qual=20, use_oq=True,
                            exclude_flags=0x400, histo='h.tsv'))
    # the parser's own errors
    for argv, message in ((['count', '-o', 'o.set'], 'at least one input is required'),
                          (['count', '-f', 'a.fq'], 'the following arguments are required: -o/--output'),
                          (['count', '-f', 'a.fq', '-o', 'o', '-u'], '-u/--use-oq: only with -b'),
                          (['count', '-f', 'a.fq', '-o', 'o', '-F', '4'], '-F/--exclude-flags: only with -b'),
                          (['count', '-f', 'a.fq', '-o', 'o', '--partitions', '65'], 'argument --partitions'),
                          (['count', '-f', 'a.fq', '-o', 'o', '--kmer-min-qual', '0'], 'argument --kmer-min-qual')):
        with pytest.raises(SystemExit) as exc:
            main.main(argv)
        assert exc.value.code == 2 and message in capsys.readouterr().err
    assert len(seen) == 4
    # the refusals of the arguments reach the user as count's ValueError, an existing -o among them
    monkeypatch.undo()
    _no_ranks(monkeypatch)
    there = tmp_path / 'there.set'
    there.write_bytes(b'kept')
    with pytest.raises(ValueError, match='exists: kbbq count does not overwrite'):
        main.main(['count', '-f', 'a.fq', '-o', str(there)])
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '2')
    from kbbq import parallel as par
    monkeypatch.setattr(par, 'init_from_env', _never)
    with pytest.raises(ValueError, match='kbbq count runs on one GPU'):
        main.main(['count', '-f', 'a.fq', '-o', str(tmp_path / 'n.set')])


def test_counts_line():
    from kbbq import kmerset
    info = dict(k=31, keep=2, inputs=2, reads=9, excluded_reads=1, windows=70, kmers=12, valley=3, partitions=1, prefilter=False,
                admitted=None, slots=1024)
    assert kmerset.count_line(info) == 'kbbq count: k=31 keep=2 inputs=2 reads=9 windows=70 kmers=12 valley=3'
    assert kmerset.count_line(dict(info, valley=None), 0x400) \
        == 'kbbq count: k=31 keep=2 inputs=2 reads=9 excluded_reads=1 windows=70 kmers=12 valley=none'
    assert kmerset.count_line(dict(info, partitions=3, kmer_min_qual=20, counted_windows=41, prefilter=True, admitted=7)) \
        == ('kbbq count: k=31 keep=2 inputs=2 reads=9 windows=70 kmers=12 valley=3 partitions=3 kmer_min_qual=20 counted_windows=41 '
            'prefilter=1 admitted=7 slots=1024')


# ---------------------------------------------------------------- the C ABI
def test_the_symbols_are_exported_declared_and_prototyped():
    import ctypes
    from kbbq import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    for name, nargs in (('kbbq_kmer_sort_pairs_bytes', 3), ('kbbq_kmer_sort_pairs_dev', 9), ('kbbq_kmer_check_pairs_dev', 12)):
        assert hasattr(lib, name) and name in N.PROTOTYPES
        ret, args = N.PROTOTYPES[name]
        assert ret is ctypes.c_int and len(args) == nargs
        declared = re.search(r'^int %s\(kbbq_ctx\* ctx,([^;]*)\);' % name, header, flags=re.M)
        assert declared and declared.group(1).count(',') == nargs - 2
    assert re.search(r'^int kbbq_kmer_check_pairs_dev\(kbbq_ctx\* ctx, const uint64_t\* d_keys, const uint32_t\* d_counts, int64_t n, int k, '
                     r'uint32_t keep,\s+int64_t first, int have_prev, uint64_t prev_key, uint64_t\* h_sums, int64_t\* bad_index, '
                     r'int\* bad_reason\);', header, flags=re.M)
    for reason, code in (('ORDER', SM.ORDER), ('RANGE', SM.RANGE), ('CANONICAL', SM.CANONICAL), ('COUNT', SM.COUNT)):
        assert re.search(r'^#define KBBQ_KMER_PAIR_%s\s+%d\s' % (reason, code), header, flags=re.M)
    from kbbq import kmer
    assert sorted(kmer.PAIR_REASONS) == [SM.ORDER, SM.RANGE, SM.CANONICAL, SM.COUNT]
    assert lib.kbbq_abi_version() == 1
    # refused on the arguments alone: no context exists without a device
    need = ctypes.c_size_t(7)
    assert lib.kbbq_kmer_sort_pairs_bytes(None, 10, ctypes.byref(need)) == N.KBBQ_E_ARG
    assert lib.kbbq_kmer_sort_pairs_dev(None, 31, None, None, None, None, 0, None, 0) == N.KBBQ_E_ARG
    index, why = ctypes.c_int64(0), ctypes.c_int(0)
    sums = np.zeros(2, dtype=np.uint64)
    assert lib.kbbq_kmer_check_pairs_dev(None, None, None, 0, 31, 2, 0, 0, 0, N.ptr(sums), ctypes.byref(index), ctypes.byref(why)) \
        == N.KBBQ_E_ARG
