"""`kbbq bqsr --kmers` on the MI355X: kbbq.gatk.bqsr.bam_to_kmer_covariates against the CPU model (tests/kmer_bqsr_model.py) -- SAM
and BAM, QUAL and OQ, with and without the prefilter, every stage of the tally's refusal chain -- and the command line: the
report byte for byte, the stderr line, `applybqsr` on that report, `bqsr -r -v` unchanged, and the refusal in a process group."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import kmer_bqsr_model as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED'):
    ENV.pop(_var, None)

_memo = {}


@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    import bamwriter
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('bqsr_kmers')
    paths = OQ.synth_bqsr_set(str(d), **B.FIXTURE)
    paths['bam'] = str(bamwriter.write_bam(d / 'aln.bam', open(paths['sam']).read()))
    reads, rgs, pus = B.load(paths['sam'])
    assert len(reads) == 600 and len(rgs) == 3
    return dict(paths=paths, reads=reads, rgs=rgs, pus=pus, dir=d)


def _want(fixture, k, t, use_oq, key='reads'):
    """The model's vectors for (k, min_count, use_oq), computed once and left unchanged; the flagged share is checked each time."""
    memo = (key, k, t, use_oq)
    if memo not in _memo:
        if (key, k, t) not in _memo:                       # the flags do not depend on which qualities are read
            _memo[(key, k, t)] = B.flags(fixture[key], k, t)
        vec, info = B.vectors(fixture[key], fixture['rgs'], k, t, use_oq=use_oq, flagged=_memo[(key, k, t)])
        for a in vec:
            a.setflags(write=False)
        _memo[memo] = (vec, info)
    vec, info = _memo[memo]
    B.check_share(info)
    return vec, info


def _same(got, want, what=''):
    assert len(got) == 9
    for name, g, w in zip(B.VEC, got, want):
        assert np.array_equal(g, w), (name, what)


CASES = [dict(k=15, min_count=None), dict(k=21, min_count=3), dict(k=15, min_count=None, use_oq=True),
         dict(k=21, min_count=3, use_oq=True), dict(k=15, min_count=None, prefilter=True), dict(k=21, min_count=3, prefilter=True, use_oq=True)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join('%s=%s' % kv for kv in c.items()))
@pytest.mark.parametrize('fused', [None, '0'])
@pytest.mark.parametrize('source', ['sam', 'bam'])
def test_vectors_equal_the_model(fixture, case, fused, source, monkeypatch):
    from kbbq import aln
    from kbbq.gatk import bqsr
    if fused is None:
        monkeypatch.delenv('KBBQ_TALLY_FUSED', raising=False)
    else:
        monkeypatch.setenv('KBBQ_TALLY_FUSED', fused)
    want, winfo = _want(fixture, case['k'], case['min_count'], case.get('use_oq', False))
    info = {}
    got = bqsr.bam_to_kmer_covariates(aln.AlignmentFile(fixture['paths'][source]), info=info, **case)
    _same(got, want, (case, fused, source))
    assert got[0].dtype == np.int64 and int(got[1].sum()) > 200 and int(got[2].sum()) > 20000
    assert info['k'] == case['k'] and info['min_count'] == winfo['min_count'] and info['reads'] == 600
    assert info['flagged_bases'] == winfo['flagged_bases']          # over all bases, soft clips included
    assert (info['admitted'] is not None) == bool(case.get('prefilter'))
    if case['k'] == 15 and case['min_count'] is None:
        assert info['min_count'] == 4                               # the first valley


def test_a_letter_outside_acgtn_runs_the_chain_down_to_character_rows(fixture, monkeypatch):
    """One forward read with an 'R' in its aligned part, among qualities below 6 so that no looked-up dinucleotide holds it:
    the fused tally and the 4-bit canonical rows refuse it (tables of their own), the character rows count it."""
    from kbbq import aln
    from kbbq.gatk import bqsr
    lines = open(fixture['paths']['sam']).read().split('\n')
    idx = 0
    hit = None
    for j, ln in enumerate(lines):
        if not ln or ln.startswith('@'):
            continue
        f = ln.split('\t')
        r = fixture['reads'][idx]
        if hit is None and not r.is_reverse and idx > 20 and r.query_alignment_start <= 20 and r.query_alignment_end >= 32:
            f[9] = f[9][:25] + 'R' + f[9][26:]
            f[10] = f[10][:25] + '$$' + f[10][27:]                      # '$' = 3 < 6
            lines[j] = '\t'.join(f)
            hit = idx
        idx += 1
    assert hit is not None
    p = fixture['dir'] / 'weird.sam'
    p.write_text('\n'.join(lines))
    reads = B.load(str(p))[0]
    assert 'R' in reads[hit].query_sequence
    fixture['weird'] = reads
    want, _ = _want(fixture, 15, None, False, key='weird')
    for fused in (None, '0'):
        if fused is None:
            monkeypatch.delenv('KBBQ_TALLY_FUSED', raising=False)
        else:
            monkeypatch.setenv('KBBQ_TALLY_FUSED', fused)
        _same(bqsr.bam_to_kmer_covariates(aln.AlignmentFile(str(p)), k=15), want, fused)


def _kbbq(*argv, timeout=300, env=None):
    return subprocess.run([sys.executable, '-m', 'kbbq.main'] + list(argv), capture_output=True, timeout=timeout, env=env or ENV)


def test_command_line_report_and_applybqsr(fixture, tmp_path):
    from kbbq.gatk import bqsr
    sam = fixture['paths']['sam']
    want, winfo = _want(fixture, 15, None, False)
    grp = tmp_path / 'kmers.grp'
    r = _kbbq('bqsr', '-b', sam, '--kmers', '-k', '15', '-g', str(grp))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == b''
    wanted = tmp_path / 'want.grp'
    bqsr.vectors_to_report(*want, fixture['pus']).write(str(wanted))
    assert grp.read_bytes() == wanted.read_bytes()
    line = 'kbbq bqsr: k=15 min_count=%d reads=600 flagged_bases=%d' % (winfo['min_count'], winfo['flagged_bases'])
    assert [ln for ln in r.stderr.decode().split('\n') if ln.startswith('kbbq bqsr:')] == [line]
    # ... with the prefilter: the same report, the longer line
    grp2 = tmp_path / 'kmers_pf.grp'
    r = _kbbq('bqsr', '-b', fixture['paths']['bam'], '--kmers', '-k', '15', '--prefilter', '-g', str(grp2))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert grp2.read_bytes() == wanted.read_bytes()
    assert re.search(r'^%s prefilter=1 admitted=\d+ slots=\d+$' % re.escape(line), r.stderr.decode(), flags=re.M)
    # applybqsr finishes the job with the code as it is
    out = tmp_path / 'recal.sam'
    r = _kbbq('applybqsr', '-b', sam, '-g', str(grp), '-o', str(out))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    before = [ln.split('\t') for ln in open(sam).read().split('\n') if ln and not ln.startswith('@')]
    after = [ln.split('\t') for ln in out.read_text().split('\n') if ln and not ln.startswith('@')]
    assert len(after) == len(before) == 600
    assert all(a[:10] + a[11:] == b[:10] + b[11:] for a, b in zip(after, before))
    assert sum(a[10] != b[10] for a, b in zip(after, before)) >= 1
    assert all(len(a[10]) == len(b[10]) for a, b in zip(after, before))


def test_bqsr_with_a_reference_is_unchanged(fixture, tmp_path):
    from kbbq import aln, benchmark
    from kbbq.gatk import bqsr
    p = fixture['paths']
    grp = tmp_path / 'ref.grp'
    r = _kbbq('bqsr', '-b', p['sam'], '-r', p['fa'], '-v', p['vcf'], '-g', str(grp))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == b'' and b'kbbq bqsr:' not in r.stderr
    wanted = tmp_path / 'want.grp'
    bqsr.bam_to_report(aln.AlignmentFile(p['sam']), p['fa'], benchmark.get_var_sites(p['vcf'])).write(str(wanted))
    assert grp.read_bytes() == wanted.read_bytes()


def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_a_process_group_is_refused_and_the_context_stays_usable(fixture, tmp_path):
    """A group of one rank (KBBQ_DIST_ALWAYS=1): the command raises its ValueError and exits non-zero; the same process then
    counts and flags the same alignments (tests/dist_bqsr_kmers_worker.py)."""
    _, winfo = _want(fixture, 15, None, False)
    grp = tmp_path / 'ranks.grp'
    env = dict(ENV, HSA_ENABLE_IPC_MODE_LEGACY='0', KBBQ_DIST_ALWAYS='1', KBBQ_DIST_BACKEND='gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
           '--master-port', str(_port()), os.path.join(ROOT, 'tests', 'dist_bqsr_kmers_worker.py'), fixture['paths']['sam'], '15', str(grp)]
    r = subprocess.run(cmd, env=env, capture_output=True, timeout=300)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode != 0
    assert re.search(r'ValueError: bqsr --kmers does not run across ranks', err), err[-3000:]
    assert 'group: initialised=True world=1' in out, (out, err[-3000:])
    assert 'afterwards: min_count=%d flagged_bases=%d' % (winfo['min_count'], winfo['flagged_bases']) in out, (out, err[-3000:])
    assert not grp.exists()
