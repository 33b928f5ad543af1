"""Static quantized qualities (--static-quantized-quals, --round-down-quantized), host side, no GPU: quantize_map against the
plain-Python model (tests/quantize_model.py), the properties of the map, the command line (what it forwards, what it refuses),
refusals before any device call or collective, and the three new symbols of the library."""
import os
import re

import numpy as np
import pytest

import quantize_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVEL_SETS = [(10, 20, 30, 40), (6,), (93,), (7, 8)]


@pytest.mark.parametrize('round_down', [False, True])
@pytest.mark.parametrize('levels', LEVEL_SETS)
def test_quantize_map_equals_the_model(levels, round_down):
    from kbbq.gatk.applybqsr import quantize_map
    got = quantize_map(levels, round_down=round_down)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (256,)
    assert got.tolist() == Q.model_map(levels, round_down)
    assert quantize_map(set(levels), round_down, 6).tolist() == got.tolist()
    assert quantize_map(list(levels) + list(levels), round_down=round_down).tolist() == got.tolist()      # a set: repeats do not matter


def test_known_values():
    """E = 6, 10, 20: q 8 is the tie between 6 and 10 and goes down; q 15 the tie between 10 and 20."""
    from kbbq.gatk.applybqsr import quantize_map
    near, down = quantize_map([10, 20]), quantize_map([10, 20], round_down=True)
    for q, n, d in [(0, 0, 0), (5, 5, 5), (6, 6, 6), (7, 6, 6), (8, 6, 6), (9, 10, 6), (10, 10, 10), (15, 10, 10), (16, 20, 10),
                    (19, 20, 10), (20, 20, 20), (41, 20, 20), (93, 20, 20), (222, 20, 20)]:
        assert (near[q + 33] - 33, down[q + 33] - 33) == (n, d), q
    assert near[:39].tolist() == list(range(39))


@pytest.mark.parametrize('levels', [(), (2, 10), (5,), (94,), (10, 94), (10.0,), (10.5,), ('10',), (None,), (True,)])
def test_invalid_levels_are_refused(levels):
    from kbbq.gatk.applybqsr import quantize_map
    with pytest.raises(ValueError):
        quantize_map(levels)
    with pytest.raises(ValueError):
        Q.model_map(levels)


def test_minscore_moves_the_floor():
    from kbbq.gatk.applybqsr import quantize_map
    assert quantize_map([2, 30], minscore=2).tolist() == Q.model_map([2, 30], minscore=2)
    with pytest.raises(ValueError):
        quantize_map([8, 30], minscore=10)


@pytest.mark.parametrize('round_down', [False, True])
@pytest.mark.parametrize('levels', LEVEL_SETS + [(6, 93), (12, 13, 14, 50)])
def test_properties_of_the_map(levels, round_down):
    from kbbq.gatk.applybqsr import quantize_map
    m = quantize_map(levels, round_down=round_down).astype(np.int64)
    E = sorted(set(levels) | {6})
    floor = 33 + 6
    assert np.array_equal(m[:floor], np.arange(floor))                       # identity below 33 + minscore
    assert np.all(np.diff(m[floor:]) >= 0)                                   # non-decreasing from there
    assert np.array_equal(m[m], m)                                           # idempotent
    assert set(m[floor:].tolist()) <= {e + 33 for e in E}                    # image within E + 33
    assert np.all(m[127:] == E[-1] + 33)                                     # q >= 94 is above every level
    assert m[0] == 0 and m[ord('!')] == ord('!')                            # padding and the row separator's neighbours stay
    if round_down:
        assert np.all(m[floor:] <= np.arange(floor, 256))


def test_a_map_of_the_wrong_kind_is_refused_by_the_entry_points(tmp_path):
    from kbbq import recalibrate
    from kbbq.gatk import applybqsr
    for bad in (np.zeros(256, np.int64), np.zeros(255, np.uint8), [1, 2, 3]):
        with pytest.raises(ValueError, match='256-byte map'):
            applybqsr.apply_report(str(tmp_path / 'absent.sam'), str(tmp_path / 'r.grp'), quantize=bad)
        with pytest.raises(ValueError, match='256-byte map'):
            recalibrate.recalibrate_fastq([str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')], quantize=bad)
        with pytest.raises(ValueError, match='256-byte map'):
            recalibrate.recalibrate_corrected(str(tmp_path / 'a.fq'), quantize=bad)
        with pytest.raises(ValueError, match='256-byte map'):
            recalibrate.recalibrate_bam(str(tmp_path / 'a.sam'), kmers={}, quantize=bad)


# ---- the command line ------------------------------------------------------------------------------------------------------------

@pytest.fixture
def cli(monkeypatch):
    """main.main with every command that takes the options recorded instead of run; any device call or collective fails."""
    from kbbq import _native, aln, main, parallel, recalibrate
    from kbbq.gatk import applybqsr
    calls = []

    def boom(*a, **kw):
        raise AssertionError('a device call or a collective was made')
    monkeypatch.setattr(_native, 'load', boom)
    for name in ('all_gather_object', 'sum_over_ranks', 'max_over_ranks', 'raise_first_error', 'barrier', 'all_to_all_rows'):
        monkeypatch.setattr(parallel, name, boom)
    monkeypatch.setattr(parallel, 'init_from_env', lambda *a, **kw: calls.append(('init',)) or (1, 0))
    monkeypatch.setattr(aln, 'AlignmentFile', lambda path: path)
    monkeypatch.setattr(recalibrate, 'check_bam_records', lambda *a, **kw: None)
    monkeypatch.setattr(recalibrate, 'check_bam_kmers', lambda *a, **kw: None)
    monkeypatch.setattr(recalibrate, 'check_corrected', lambda *a, **kw: None)
    info = dict(k=31, min_count=4, reads=6, flagged_bases=7, changed_bases=7, slots=64)
    monkeypatch.setattr(recalibrate, 'recalibrate', lambda **kw: calls.append(('two', kw)))
    monkeypatch.setattr(recalibrate, 'recalibrate_corrected', lambda path, **kw: calls.append(('one', dict(kw, path=path))) or dict(info))
    monkeypatch.setattr(recalibrate, 'recalibrate_bam', lambda bam, **kw: calls.append(('bam', dict(kw, bam=bam))) or dict(info))
    monkeypatch.setattr(applybqsr, 'apply_report', lambda *a, **kw: calls.append(('apply', kw)))
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                # the command then leaves the memory back end alone
    return main, calls


COMMANDS = [('two', ['recalibrate', '-f', 'a.fq', 'b.fq']), ('one', ['recalibrate', '-c', 'a.fq']),
            ('bam', ['recalibrate', '-b', 'a.sam', '--kmers']), ('apply', ['applybqsr', '-b', 'a.sam', '-g', 'r.grp'])]


@pytest.mark.parametrize('which,argv', COMMANDS)
def test_the_parser_forwards_the_map(cli, capsys, which, argv):
    main, calls = cli
    main.main(argv + ['--static-quantized-quals', '10,20', '--static-quantized-quals', '30', '--static-quantized-quals', '20,40'])
    got = [c for c in calls if c[0] == which]
    assert len(got) == 1 and got[0][1]['quantize'].tolist() == Q.model_map([10, 20, 30, 40])
    del calls[:]
    main.main(argv + ['--round-down-quantized', '--static-quantized-quals', '10, 20'])
    got = [c for c in calls if c[0] == which]
    assert got[0][1]['quantize'].tolist() == Q.model_map([10, 20], round_down=True)
    capsys.readouterr()


@pytest.mark.parametrize('which,argv', COMMANDS)
def test_without_the_option_the_call_is_the_one_it_was(cli, capsys, which, argv):
    main, calls = cli
    main.main(argv)
    got = [c for c in calls if c[0] == which]
    assert len(got) == 1 and 'quantize' not in got[0][1]
    capsys.readouterr()


@pytest.mark.parametrize('which,argv', COMMANDS)
@pytest.mark.parametrize('more,said', [
    (['--round-down-quantized'], '--round-down-quantized: only with --static-quantized-quals'),
    (['--static-quantized-quals', '5'], 'levels must be in 6..93, got 5'),
    (['--static-quantized-quals', '10,94'], 'levels must be in 6..93, got 94'),
    (['--static-quantized-quals', '10', '--static-quantized-quals', '2'], 'levels must be in 6..93, got 2'),
    (['--static-quantized-quals', '10.5'], 'is not an integer'),
    (['--static-quantized-quals', 'ten'], 'is not an integer'),
    (['--static-quantized-quals', ''], 'is not an integer'),
    (['--static-quantized-quals', '10,,20'], 'is not an integer'),
    (['--static-quantized-quals', '10,'], 'is not an integer'),
    (['--static-quantized-quals'], 'expected one argument'),
])
def test_argparse_errors_come_before_the_device_and_before_any_collective(cli, capsys, which, argv, more, said):
    """The fixture fails any library load or collective, and records parallel.init_from_env: the parser has refused before
    the command joins a process group."""
    main, calls = cli
    with pytest.raises(SystemExit) as e:
        main.main(argv + more)
    assert e.value.code == 2 and not calls
    assert said in capsys.readouterr().err


def test_other_commands_do_not_take_the_option(cli, capsys):
    main, calls = cli
    for argv in (['correct', '-f', 'a.fq'], ['bqsr', '-b', 'a.sam', '--kmers', '-g', 'r.grp']):
        with pytest.raises(SystemExit):
            main.main(argv + ['--static-quantized-quals', '10'])
    assert not calls
    capsys.readouterr()


def test_refusals_of_the_functions_arrive_with_no_device_and_no_collective(monkeypatch, tmp_path):
    """quantize_map and the entry points' check of the map run on the host alone, on every rank."""
    from kbbq import _native, kmer, parallel, recalibrate
    from kbbq.gatk import applybqsr

    def boom(*a, **kw):
        raise AssertionError('a device call or a collective was made')
    monkeypatch.setattr(_native, 'load', boom)
    monkeypatch.setattr(kmer, '_ctx', boom)
    for name in ('all_gather_object', 'sum_over_ranks', 'max_over_ranks', 'raise_first_error', 'barrier', 'all_to_all_rows',
                 'init_from_env'):
        monkeypatch.setattr(parallel, name, boom)
    for rank in (0, 1):
        monkeypatch.setattr(parallel, 'world_rank', lambda rank=rank: (2, rank))
        with pytest.raises(ValueError):
            applybqsr.quantize_map([])
        with pytest.raises(ValueError):
            applybqsr.quantize_map([3])
        with pytest.raises(ValueError, match='256-byte map'):
            applybqsr.apply_report(str(tmp_path / 'absent.sam'), str(tmp_path / 'r.grp'), output=str(tmp_path / 'o.sam'),
                                   quantize=np.zeros(3, np.uint8))
        with pytest.raises(ValueError, match='256-byte map'):
            recalibrate.recalibrate(None, [str(tmp_path / 'a.fq'), str(tmp_path / 'b.fq')], quantize=np.zeros(3, np.uint8))
    assert not os.listdir(tmp_path)


# ---- the library ------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_declared():
    from kbbq import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, 'include', 'kbbq_hip.h')).read()
    for name in ('kbbq_quantize_plane_dev', 'kbbq_apply_aligned_q_dev', 'kbbq_apply_aligned_q'):
        assert hasattr(lib, name) and name in N.PROTOTYPES
        assert re.search(r'\bint\s+%s\(' % name, header)
    assert len(N.PROTOTYPES['kbbq_apply_aligned_q_dev'][1]) == len(N.PROTOTYPES['kbbq_apply_aligned_dev'][1]) + 1
    assert len(N.PROTOTYPES['kbbq_apply_aligned_q'][1]) == len(N.PROTOTYPES['kbbq_apply_aligned'][1]) + 1
    assert lib.kbbq_abi_version() == 1
