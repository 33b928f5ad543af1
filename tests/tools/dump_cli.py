#!/usr/bin/env python3
"""The command line as text, to compare two trees with `diff`: no device, no input files.

    python tests/tools/dump_cli.py             every action of every sub-command: option strings, dest, type, default, metavar,
                                               nargs, action class, required, help
    python tests/tools/dump_cli.py --refusals  the exit status and stderr of misplaced-flag command lines (from the host tests'
                                               parametrize lists, plus lines that misplace flags of several groups at once)

The parser comes from kbbq.main.build_parser(); on a tree without it, from the parse_args call main() makes."""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))
from kbbq import main                                               # noqa: E402


def the_parser():
    if hasattr(main, 'build_parser'):
        return main.build_parser()[0]

    class Caught(Exception):
        pass

    def parse_args(self, *a, **kw):
        raise Caught(self)
    real, argparse.ArgumentParser.parse_args = argparse.ArgumentParser.parse_args, parse_args
    try:
        main.main([])
    except Caught as caught:
        return caught.args[0]
    finally:
        argparse.ArgumentParser.parse_args = real


def dump_actions():
    parser = the_parser()
    commands = next(a for a in parser._actions if isinstance(a, argparse._SubParsersAction)).choices
    for name, sub in commands.items():
        print('== %s: %s' % (name, sub.description))
        for a in sub._actions:
            print('%s | dest=%s type=%s default=%r metavar=%r nargs=%r action=%s required=%r\n    %s'
                  % (' '.join(a.option_strings), a.dest, getattr(a.type, '__name__', a.type), a.default, a.metavar, a.nargs,
                     type(a).__name__, a.required, a.help))


_RECAL_F = ['recalibrate', '-f', 'a.fq', 'b.fq']
_BQSR = ['bqsr', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf', '-g', 'r']
_BENCH = ['benchmark', '-b', 'x', '-r', 'x.fa', '-v', 'x.vcf']
REFUSED = [
    _RECAL_F + ['--kmers-from', 's'],
    ['recalibrate', '-b', 'a.bam', '--kmers-from', 's'],
    _BQSR + ['--kmers-from', 's'],
    _BENCH + ['--kmers-from', 's'],
    ['correct', '-f', 'a.fq', '--kmers-from', 's', '--prefilter', '--partitions', '2', '--local-slots', '64'],
    ['recalibrate', '-c', 'a.fq', '--kmers-from', 's', '--filter-bits', '4', '--kmer-min-qual', '20'],
    ['count', '-f', 'a.fq', '-o', 'o', '-u'],
    ['count', '-f', 'a.fq', '-o', 'o', '-F', '4'],
    ['count', '-f', 'a.fq', '-o', 'o', '-u', '-F', '4'],
    ['count', '-o', 'o'],
    ['count', '-f', 'a.fq'],
    _BQSR + ['--skip-unresolved'],
    _RECAL_F + ['--skip-unresolved'],
    _RECAL_F + ['--passes', '2'],
    _BQSR + ['--passes', '2'],
    _BENCH + ['--passes', '2'],
    _BENCH + ['-k', '21'],
    _BENCH + ['--min-count', '3'],
    _BENCH + ['--slots', '1024'],
    _BENCH + ['-f', 'x.fq', '--prefilter', '--filter-bits', '4'],
    _BENCH + ['--kmers', '-f', 'x.fq'],
    _RECAL_F + ['--fix-n'],
    _BQSR + ['--mixed-lengths'],
    _BQSR + ['-F', '0xF00'],
    ['bqsr', '-b', 'x', '-g', 'r', '--mixed-lengths', '--exclude-flags', '4'],
    ['bqsr', '-b', 'x', '-g', 'r', '--kmers', '-r', 'x.fa', '-v', 'x.vcf'],
    ['bqsr', '-b', 'x', '-g', 'r'],
    _BQSR + ['-k', '21', '--slots', '64', '-u', '--partitions', '2', '-F', '4', '--kmer-min-qual', '20'],
    ['recalibrate', '-b', 'x.bam', '--mixed-lengths'],
    ['recalibrate', '-c', 'x.fq', '--mixed-lengths'],
    _RECAL_F + ['-F', '4'],
    _RECAL_F + ['--kmers', '--mixed-lengths'],
    _RECAL_F + ['--kmer-min-qual', '20'],
    ['recalibrate', '-b', 'a.bam', '--kmer-min-qual', '20'],
    _RECAL_F + ['--partitions', '2'],
    _BQSR + ['--partitions', '2'],
    _RECAL_F + ['--kmers'],
    ['recalibrate', '-c', 'x.fq', '--kmers'],
    ['recalibrate', '-b', 'x.bam', '--kmers', '--fix-n', '--infer-rg'],
    ['recalibrate', '-b', 'x.bam', '-k', '21'],
    ['recalibrate', '-b', 'x.bam', '--min-count', '3', '--slots', '64', '--prefilter', '--passes', '2', '--skip-unresolved',
     '--partitions', '2'],
    ['recalibrate', '-b', 'x.bam', '--round-down-quantized'],
    ['recalibrate', '-b', 'x.bam', '--kmers', '--bam-out', '--bgzf'],
    ['recalibrate', '-c', 'x.fq', '--bam-out'],
    # flags of several groups at once: the group refused first
    _RECAL_F + ['--kmers-from', 's', '--mixed-lengths', '--kmer-min-qual', '20', '--kmers', '-k', '21'],
    _RECAL_F + ['--mixed-lengths', '--kmer-min-qual', '20', '--kmers', '-k', '21'],
    _RECAL_F + ['--kmer-min-qual', '20', '--kmers', '-k', '21'],
    _RECAL_F + ['--bam-out', '--mixed-lengths'],
    _BQSR + ['--kmers-from', 's', '-k', '21'],
    # the one accepted difference: --passes before --skip-unresolved
    _BQSR + ['--skip-unresolved', '--passes', '2'],
]


def dump_refusals():
    for argv in REFUSED:
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            try:
                main.main(list(argv))
                status = 'returned'
            except SystemExit as e:
                status = 'exit %r' % (e.code,)
            except Exception as e:                                  # noqa: BLE001 -- a command line that got past the parser
                status = '%s: %s' % (type(e).__name__, e)
        print('$ kbbq %s\n%s\n%s' % (' '.join(argv), status, err.getvalue().rstrip('\n').rsplit('\n', 1)[-1]))


if __name__ == '__main__':
    dump_refusals() if sys.argv[1:] == ['--refusals'] else dump_actions()
