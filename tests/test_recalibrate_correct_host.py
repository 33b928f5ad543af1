"""`kbbq recalibrate -c`, host side, no GPU: the four new entry points are exported and bound as the header declares them, the
command line takes the new source and its options, and what the one-file path refuses it refuses before any device call or
collective."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_vp, _i, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
NEW = {
    # ctx, table, d_seq, d_meta, nrows, pitch, flags
    'kbbq_kmer_count_rows_dev': [_vp, _vp, _vp, _vp, _i64, _i, _i],
    # ctx, filter, k, d_seq, d_meta, nrows, pitch, flags
    'kbbq_kmer_prefilter_rows_dev': [_vp, _vp, _i, _vp, _vp, _i64, _i, _i],
    # ctx, table, filter, d_seq, d_meta, nrows, pitch, flags
    'kbbq_kmer_count_filtered_rows_dev': [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i],
    # ctx, table, d_seq, d_meta, nrows, pitch, flags, min_count, d_out, d_changed
    'kbbq_kmer_correct_rows_dev': [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp],
}


def _header_types(name):
    """ctypes of the parameters of `name` as include/kbbq_hip.h declares it: pointers, int64_t, int."""
    with open(os.path.join(ROOT, 'include', 'kbbq_hip.h')) as fh:
        text = fh.read()
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, text, re.S)
    assert m, '%s is not declared in the header' % name
    out = []
    for param in m.group(1).split(','):
        param = ' '.join(param.split())
        out.append(_vp if '*' in param else _i64 if param.startswith('int64_t') else _i if param.startswith('int ') else None)
    return out


@pytest.mark.parametrize('name', sorted(NEW))
def test_new_symbols_are_exported_and_bound(name):
    from kbbq import _native as N
    lib = N.load()
    fn = getattr(lib, name)                                  # AttributeError when the library lacks it
    res, args = N.PROTOTYPES[name]
    assert res is _i and args == NEW[name] == _header_types(name)
    assert fn.restype is _i and list(fn.argtypes) == NEW[name]


def test_abi_version_is_still_one():
    from kbbq import _native as N
    assert N.load().kbbq_abi_version() == 1


def test_bad_flags_are_refused_without_a_device():
    from kbbq import _native as N
    lib = N.load()
    assert lib.kbbq_kmer_count_rows_dev(None, None, None, None, 0, 16, 8) == N.KBBQ_E_ARG
    assert lib.kbbq_kmer_correct_rows_dev(None, None, None, None, 0, 16, N.ROWS_TWINS, 2, None, None) == N.KBBQ_E_ARG
    assert lib.kbbq_kmer_count_rows_dev(None, None, None, None, 0, 16, N.ROWS_NIBBLES) == N.KBBQ_E_ARG     # NULL ctx / table


@pytest.fixture
def cli(monkeypatch):
    """main.main with both recalibrate paths recorded instead of run."""
    from kbbq import main, recalibrate
    calls = []
    monkeypatch.setattr(recalibrate, 'recalibrate', lambda **kw: calls.append(('two', kw)))
    monkeypatch.setattr(recalibrate, 'recalibrate_corrected',
                        lambda path, **kw: calls.append(('one', dict(kw, path=path))) or
                        dict(k=kw['k'], min_count=4, reads=10, changed_bases=7, slots=2048, admitted=99))
    monkeypatch.setattr(recalibrate, 'check_corrected', lambda *a, **kw: None)
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                # the command then leaves the memory back end alone
    return main, calls


def test_argparse_takes_the_new_source_and_options(cli, capsys):
    main, calls = cli
    main.main(['recalibrate', '-f', 'a.fq', 'b.fq'])
    main.main(['recalibrate', '-f', 'a.fq', 'b.fq', '-g', 'm.grp', '--infer-rg', '-o', 'out.fq'])
    assert calls[0] == ('two', dict(bam=None, fastq=['a.fq', 'b.fq'], infer_rg=False, use_oq=False, set_oq=False, gatkreport=None,
                                    output=None))
    assert calls[1][1]['fastq'] == ['a.fq', 'b.fq'] and calls[1][1]['gatkreport'] == 'm.grp' and calls[1][1]['output'] == 'out.fq'
    assert capsys.readouterr().err == ''
    main.main(['recalibrate', '-c', 'x.fq'])
    assert calls[2] == ('one', dict(path='x.fq', infer_rg=False, gatkreport=None, output=None, k=31, min_count=None, slots=None,
                                    prefilter=False, filter_bits=4))
    assert capsys.readouterr().err == 'kbbq recalibrate: k=31 min_count=4 reads=10 changed_bases=7\n'
    main.main(['recalibrate', '--correct', 'x.fq', '-k', '21', '--min-count', '3', '--slots', '4096', '--prefilter', '--filter-bits',
               '8', '--infer-rg', '-g', 'm.grp', '-o', 'o.fq'])
    assert calls[3] == ('one', dict(path='x.fq', infer_rg=True, gatkreport='m.grp', output='o.fq', k=21, min_count=3, slots=4096,
                                    prefilter=True, filter_bits=8))
    assert capsys.readouterr().err == 'kbbq recalibrate: k=21 min_count=4 reads=10 changed_bases=7 prefilter=1 admitted=99 slots=2048\n'


@pytest.mark.parametrize('argv', [
    ['-c', 'x.fq', '-f', 'a.fq', 'b.fq'], ['-c', 'x.fq', '-b', 'x.bam'], ['-f', 'a.fq', 'b.fq', '-b', 'x.bam'], [],
    ['-f', 'a.fq', 'b.fq', '-k', '21'], ['-f', 'a.fq', 'b.fq', '--min-count', '3'], ['-f', 'a.fq', 'b.fq', '--slots', '1024'],
    ['-f', 'a.fq', 'b.fq', '--prefilter'], ['-b', 'x.bam', '--filter-bits', '4'], ['-f', 'a.fq'], ['-c'], ['-c', 'x.fq', 'y.fq'],
])
def test_argparse_errors(cli, argv, capsys):
    main, calls = cli
    with pytest.raises(SystemExit) as e:
        main.main(['recalibrate'] + argv)
    assert e.value.code == 2 and not calls
    capsys.readouterr()


@pytest.fixture
def no_device(monkeypatch):
    """Every way into the device, the files and the collectives fails the test."""
    from kbbq import _device, _native, fastx, kmer, parallel, recalibrate

    def boom(*a, **kw):
        raise AssertionError('a device call, a collective or a read of the input was made')
    monkeypatch.setattr(_native, 'load', boom)
    for mod, names in ((kmer, ('_ctx', 'prefilter_batch', 'count_batch', 'correct_batch', 'KmerTable', 'KmerFilter')),
                       (_device, ('context', 'warm_up', 'device_budget', 'use_native_memory')),
                       (fastx, ('PairScan', 'pack_single', 'NativeFastq')),
                       (recalibrate, ('_warm_up', '_tally_local')),
                       (parallel, ('init_from_env', 'all_gather_object', 'broadcast_object', 'raise_first_error', 'barrier',
                                   'allreduce_tables', 'in_rank_order'))):
        for name in names:
            monkeypatch.setattr(mod, name, boom)
    monkeypatch.setattr(kmer, '_ranks', lambda: None)
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_SEQUENTIAL', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)
    return recalibrate


@pytest.fixture
def fq(tmp_path):
    p = tmp_path / 'reads.fq'
    p.write_text('@r1\nACGT\n+\nIIII\n')
    return str(p)


def _both(recalibrate, match, argv, **kw):
    """The API and the command line refuse alike, with a ValueError that names the two-command form where there is one."""
    from kbbq import main
    path = kw.pop('path')
    with pytest.raises(ValueError, match=match) as e:
        recalibrate.recalibrate_corrected(path, **kw)
    with pytest.raises(ValueError, match=match):
        main.main(['recalibrate', '-c', path] + argv)
    return str(e.value)


@pytest.mark.parametrize('world,rank', [(2, 0), (2, 1), (8, 5)])
def test_ranks_are_refused_before_any_collective(no_device, fq, monkeypatch, world, rank):
    from kbbq import kmer
    monkeypatch.setattr(kmer, '_ranks', lambda: (world, rank))
    msg = _both(no_device, 'ranks', [], path=fq)
    assert 'kbbq correct -f' in msg and 'kbbq recalibrate -f' in msg


@pytest.mark.parametrize('world,rank', [(2, 0), (2, 1)])
def test_a_launcher_is_refused_before_the_process_group(no_device, fq, monkeypatch, world, rank):
    monkeypatch.setenv('RANK', str(rank))
    monkeypatch.setenv('WORLD_SIZE', str(world))
    msg = _both(no_device, 'ranks', [], path=fq)
    assert 'kbbq correct -f' in msg and 'kbbq recalibrate -f' in msg


def test_pipes_and_standard_input_are_refused(no_device, tmp_path):
    fifo = str(tmp_path / 'reads.fifo')
    os.mkfifo(fifo)
    for path in (fifo, '-'):
        if path == '-':
            with pytest.raises(ValueError, match='mapped') as e:
                no_device.recalibrate_corrected(path)
            msg = str(e.value)
        else:
            msg = _both(no_device, 'mapped', [], path=path)
        assert 'kbbq correct -f' in msg and 'kbbq recalibrate -f' in msg


def test_sequential_reading_is_refused(no_device, fq, monkeypatch, tmp_path):
    monkeypatch.setenv('KBBQ_SEQUENTIAL', '1')
    msg = _both(no_device, 'KBBQ_SEQUENTIAL', [], path=fq)
    assert 'kbbq correct -f' in msg and 'kbbq recalibrate -f' in msg
    monkeypatch.delenv('KBBQ_SEQUENTIAL')
    import gzip
    gz = str(tmp_path / 'reads.fq.gz')
    with gzip.open(gz, 'wb') as fh:
        fh.write(b'@r1\nACGT\n+\nIIII\n')
    monkeypatch.setenv('KBBQ_GZ_STREAM_BYTES', '16')         # this .gz file is then one the mapped path does not take
    _both(no_device, 'KBBQ_GZ_STREAM_BYTES', [], path=gz)


def test_an_existing_report_is_refused(no_device, fq, tmp_path):
    grp = tmp_path / 'model.grp'
    grp.write_text('#:GATKReport.v1.1:5\n')
    _both(no_device, 'exists', ['-g', str(grp)], path=fq, gatkreport=str(grp))


def test_the_prefilter_and_the_k_mer_options_are_checked(no_device, fq):
    _both(no_device, 'min_count', ['--prefilter', '--min-count', '1'], path=fq, prefilter=True, min_count=1)
    _both(no_device, 'filter_bits', ['--prefilter', '--filter-bits', '0'], path=fq, prefilter=True, filter_bits=0)
    _both(no_device, 'filter_bits', ['--prefilter', '--filter-bits', '65'], path=fq, prefilter=True, filter_bits=65)
    _both(no_device, 'k must be', ['-k', '7'], path=fq, k=7)
    _both(no_device, 'k must be', ['-k', '33'], path=fq, k=33)
    _both(no_device, 'min_count', ['--min-count', '0'], path=fq, min_count=0)
