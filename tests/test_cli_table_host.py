"""The command line's two tables without a GPU (kbbq/main.py _KMER_OPTIONS, _COMMANDS): which k-mer flags each command offers,
that every one of them comes from the option table, and kmer.summary_line against the stderr lines the four commands printed
before there was one function for them."""
import inspect

import pytest

# command x flag, written from the command line as it was before the tables: the k-mer flags and no others
K, COUNT, SLOTS, PRE, BITS = '-k/--kmer', '--min-count', '--slots', '--prefilter', '--filter-bits'
FIXN, PASSES, SKIP, PARTS = '--fix-n', '--passes', '--skip-unresolved', '--partitions'
MIXED, EXCL, MINQ, FROM, LOCAL = '--mixed-lengths', '-F/--exclude-flags', '--kmer-min-qual', '--kmers-from', '--local-slots'
EVERY = (K, COUNT, SLOTS, PRE, BITS, FIXN, PASSES, SKIP, PARTS, MIXED, EXCL, MINQ, FROM, LOCAL)
OFFERED = {
    'help': (),
    'recalibrate': (K, COUNT, SLOTS, PRE, BITS, FIXN, PASSES, SKIP, PARTS, MIXED, EXCL, MINQ, FROM),
    'benchmark': (K, COUNT, SLOTS, PRE, BITS, PASSES, PARTS, MINQ, FROM),
    'applybqsr': (),
    'bqsr': (K, COUNT, SLOTS, PRE, BITS, PASSES, SKIP, PARTS, MIXED, EXCL, MINQ, FROM),
    'correct': (K, COUNT, SLOTS, PRE, BITS, FIXN, PASSES, PARTS, MINQ, FROM, LOCAL),
    'count': (K, SLOTS, PRE, BITS, PARTS, MINQ, EXCL),
}


def test_every_command_offers_its_kmer_flags_and_no_others():
    import argparse
    from kbbq import main
    parser, parsers = main.build_parser()
    commands = next(a for a in parser._actions if isinstance(a, argparse._SubParsersAction)).choices
    assert set(commands) == set(OFFERED) and set(parsers) == set(OFFERED) - {'help'}
    for name, sub in commands.items():
        offered = {'/'.join(a.option_strings) for a in sub._actions} & set(EVERY)
        assert offered == set(OFFERED[name]), name
        assert name == 'help' or parsers[name] is sub


def test_every_kmer_flag_is_declared_once_in_the_option_table():
    from kbbq import main
    assert tuple('/'.join(flags) for flags, _, _ in main._KMER_OPTIONS.values()) == EVERY
    source = inspect.getsource(main)
    for flag in (f for both in EVERY for f in both.split('/')):
        assert source.count(repr(flag)) == 1, flag
    # ... and what a command's row names is what _add_kmer_options gave it
    for name, row in main._COMMANDS.items():
        assert {'/'.join(main._KMER_OPTIONS[dest][0]) for dest in row['options']} == set(OFFERED[name]), name


ON = dict(k=21, min_count=3, reads=1000, excluded_reads=7, changed_bases=55, flagged_bases=66, skipped_bases=5, partitions=4,
          kmer_min_qual=20, counted_windows=12345, admitted=99, slots=2048, kmers_from=True, loaded_kmers=777)
OFF = dict(k=31, min_count=2, reads=10, changed_bases=0, flagged_bases=1, slots=64)


@pytest.mark.parametrize('command,info,options,bases,line', [
    ('correct', ON, dict(fix_n=True, passes=3, prefilter=True), 'changed_bases',
     'kbbq correct: k=21 min_count=3 reads=1000 changed_bases=55 fix_n=1 passes=3 partitions=4 kmer_min_qual=20 '
     'counted_windows=12345 prefilter=1 admitted=99 slots=2048 kmers_from=1 loaded_kmers=777\n'),
    ('recalibrate', OFF, dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4), 'changed_bases',
     'kbbq recalibrate: k=31 min_count=2 reads=10 changed_bases=0\n'),
    ('recalibrate', ON, dict(k=31, min_count=None, slots=None, prefilter=True, filter_bits=4, exclude_flags=0x400, skip_unresolved=True,
                             passes=3, partitions=4, kmer_min_qual=20), 'flagged_bases',
     'kbbq recalibrate: k=21 min_count=3 reads=1000 excluded_reads=7 flagged_bases=66 skipped_bases=5 passes=3 partitions=4 '
     'kmer_min_qual=20 counted_windows=12345 prefilter=1 admitted=99 slots=2048 kmers_from=1 loaded_kmers=777\n'),
    ('bqsr', OFF, dict(k=31, min_count=None, slots=None, prefilter=False, filter_bits=4, passes=1), 'flagged_bases',
     'kbbq bqsr: k=31 min_count=2 reads=10 flagged_bases=1\n'),
])
def test_the_summary_line_is_the_one_each_command_printed(command, info, options, bases, line):
    """The literal lines are the commands' stderr, byte for byte, from before kmer.summary_line; `options`: the keywords the
    command collects for such a command line."""
    from kbbq import kmer
    assert kmer.summary_line(command, info, options, bases) == line
