"""`kbbq recalibrate -b ALN --kmers` on the MI355X: stdout, `-o`, the `-g` report and the stderr line against `kbbq bqsr --kmers -g R`
followed by `kbbq applybqsr -g R`, run in the same test on the same file -- SAM and BAM, every option -- on
kmer_bqsr_model.FIXTURE as written (every record carries an OQ tag), with the tags of every other record removed (the OQ plane
then follows SEQ and QUAL for the context) and with all of them removed; that the fixture is not degenerate; what went to the
device (recalibrate.LAST_RUN['aligned'], and how often the reader filled each plane); the tally's chain down to character
rows; the command as a process of its own, without torch; and the refusal in a process group."""
import os
import re
import socket
import subprocess
import sys

import pytest

import kmer_bqsr_model as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'))
for _var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED'):
    ENV.pop(_var, None)


def _without_oq(text, keep):
    """The SAM text with the OQ tag removed from every record i for which keep(i) is false."""
    out, i = [], 0
    for ln in text.split('\n'):
        if ln and not ln.startswith('@'):
            if not keep(i):
                ln = '\t'.join(f for f in ln.split('\t') if not f.startswith('OQ:Z:'))
            i += 1
        out.append(ln)
    return '\n'.join(out)


@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    import bamwriter
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('recalibrate_bam')
    sam = OQ.synth_bqsr_set(str(d), **B.FIXTURE)['sam']
    text = open(sam).read()
    texts = dict(all=text, half=_without_oq(text, lambda i: i % 2 == 0), none=_without_oq(text, lambda i: False))
    paths = {}
    for name, t in texts.items():
        p = d / ('%s.sam' % name)
        p.write_text(t)
        paths[name, 'sam'] = str(p)
        paths[name, 'bam'] = str(bamwriter.write_bam(d / ('%s.bam' % name), t))
    reads = B.load(sam)[0]
    assert len(reads) == 600 and text.count('OQ:Z:') == 600 and texts['half'].count('OQ:Z:') == 300 and 'OQ:Z:' not in texts['none']
    return dict(paths=paths, texts=texts, reads=reads, dir=d)


@pytest.fixture
def kbbq(monkeypatch, capfdbinary):
    """The command line in this process: main.main(argv) -> (stdout bytes, its `kbbq ...:` lines of stderr)."""
    from kbbq import main
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                      # this process has torch tensors already
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS', 'KBBQ_TALLY_FUSED'):
        monkeypatch.delenv(var, raising=False)

    def run(*argv):
        capfdbinary.readouterr()
        main.main([str(a) for a in argv])
        sys.stdout.flush()
        sys.stderr.flush()
        out, err = capfdbinary.readouterr()
        return out, [ln for ln in err.decode().split('\n') if ln.startswith('kbbq ')]
    return run


def _records(text):
    if isinstance(text, bytes):
        text = text.decode('latin-1')
    return [ln.split('\t') for ln in text.split('\n') if ln and not ln.startswith('@')]


def _line(said):
    """The one `kbbq ...:` line of a run, with the two figures that are not reproducible made equal: the prefilter's `admitted` counts
    the k-mers whose filter bits were all set when a thread got to them, which depends on the order in which the threads of
    the launch arrive -- two runs of `kbbq bqsr --kmers --prefilter` on one file print different numbers (1713 and 1716 here) -- and
    the default `slots` is sized from it.  Everything else in the line, and every byte of the outputs, is compared as it is."""
    assert len(said) == 1, said
    return re.sub(r' admitted=\d+ slots=\d+$', ' admitted=# slots=#', said[0])


K15 = ('-k', '15')
# (id, the records' OQ tags, k-mer options, -u / -s)
CASES = [
    ('plain', 'all', K15, ()),
    ('plain-no-oq', 'none', K15, ()),
    ('plain-half-oq', 'half', K15, ()),
    ('u', 'all', K15, ('-u',)),
    ('s', 'half', K15, ('-s',)),
    ('u-s', 'all', K15, ('-u', '-s')),
    ('min-count-3-k-21', 'half', ('--min-count', '3', '-k', '21'), ()),
    ('prefilter', 'half', K15 + ('--prefilter',), ()),
    ('skip-unresolved', 'half', K15 + ('--skip-unresolved',), ()),
    ('passes-2', 'half', K15 + ('--passes', '2'), ()),
    ('partitions-3', 'half', K15 + ('--partitions', '3'), ()),
    ('all-of-these', 'all', ('--min-count', '3', '-k', '21', '--prefilter', '--skip-unresolved', '--passes', '2', '--partitions', '3'),
     ('-u', '-s')),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize('source', ['sam', 'bam'])
def test_the_bytes_are_those_of_the_two_commands(fixture, kbbq, tmp_path, source, case):
    _, oq, kopts, us = case
    aln = fixture['paths'][oq, source]
    u = tuple(x for x in us if x == '-u')
    grp, want_out = tmp_path / 'two.grp', tmp_path / 'two.sam'
    out, said = kbbq('bqsr', '-b', aln, '--kmers', *kopts, *u, '-g', grp)
    assert out == b'' and _line(said).startswith('kbbq bqsr: k=')
    want_line = 'kbbq recalibrate:' + _line(said)[len('kbbq bqsr:'):]
    want, said = kbbq('applybqsr', '-b', aln, '-g', grp, *us)
    assert said == [] and len(_records(want)) == 600
    assert kbbq('applybqsr', '-b', aln, '-g', grp, *us, '-o', want_out) == (b'', [])
    assert want_out.read_bytes() == want

    got, said = kbbq('recalibrate', '-b', aln, '--kmers', *kopts, *us)
    assert _line(said) == want_line
    assert got == want
    mine, one_out = tmp_path / 'one.grp', tmp_path / 'one.sam'
    got, said = kbbq('recalibrate', '-b', aln, '--kmers', *kopts, *us, '-g', mine, '-o', one_out)
    assert got == b'' and _line(said) == want_line
    assert one_out.read_bytes() == want
    assert mine.read_bytes() == grp.read_bytes()
    # no @PG line, the header as read
    head = [ln for ln in fixture['texts'][oq].split('\n') if ln.startswith('@')]
    assert [ln for ln in want.decode().split('\n') if ln.startswith('@')] == head
    for opt, field in (('--skip-unresolved', ' skipped_bases='), ('--passes', ' passes=2'), ('--partitions', ' partitions=3'),
                       ('--prefilter', ' prefilter=1 admitted=# slots=#')):
        assert (field in want_line) == (opt in kopts), want_line


def test_the_fixture_is_not_degenerate(fixture, kbbq):
    """The model flags 1..10 % of the bases (and the command counts the same bases), qualities change, and with -s every changed
    record without an OQ tag gains one that holds its QUAL as read -- and no record that has one changes its tags."""
    err, t = B.flags(fixture['reads'], 15)
    info = dict(min_count=t, flagged_bases=int(err.sum()), bases=600 * 60)
    B.check_share(info)
    got, said = kbbq('recalibrate', '-b', fixture['paths']['half', 'sam'], '--kmers', '-k', '15', '-s')
    assert said == ['kbbq recalibrate: k=15 min_count=%d reads=600 flagged_bases=%d' % (t, info['flagged_bases'])]
    before, after = _records(fixture['texts']['half']), _records(got)
    assert len(before) == len(after) == 600
    changed = gained = 0
    for i, (b, a) in enumerate(zip(before, after)):
        assert a[:10] == b[:10] and len(a[10]) == len(b[10]) == 60
        had = any(f.startswith('OQ:Z:') for f in b[11:])
        assert had == (i % 2 == 0)
        if a[10] != b[10]:
            changed += 1
        if not had:                                   # (`applybqsr -s` adds the tag to an unchanged record too)
            assert a[11:] == b[11:] + ['OQ:Z:' + b[10]]
            gained += a[10] != b[10]
        else:
            assert a[11:] == b[11:]
    assert changed >= 1 and gained >= 1, (changed, gained)
    # without -s the same qualities and no tag anywhere
    plain, _ = kbbq('recalibrate', '-b', fixture['paths']['half', 'sam'], '--kmers', '-k', '15')
    assert [r[:11] for r in _records(plain)] == [r[:11] for r in after]
    assert all(p[11:] == b[11:] for p, b in zip(_records(plain), before))


@pytest.mark.parametrize('source', ['sam', 'bam'])
@pytest.mark.parametrize('oq,use_oq,planes', [('none', False, ['SEQ', 'QUAL']), ('all', True, ['SEQ', 'OQ']),
                                              ('half', False, ['SEQ', 'QUAL', 'OQ']), ('all', False, ['SEQ', 'QUAL', 'OQ'])],
                         ids=['plain', 'u', 'half-oq', 'all-oq-plain'])
def test_every_plane_is_filled_and_uploaded_once(fixture, monkeypatch, tmp_path, source, oq, use_oq, planes):
    """LAST_RUN['aligned'] names what went to the device: SEQ and the source qualities, n x pitch x 2 bytes; a third plane only where
    records carry OQ tags that are not the source (`applybqsr` takes their context from the tag).  The reader fills each once."""
    from kbbq import aln, recalibrate
    filled = []
    plane = aln.SamBatch.plane

    def counted(self, which, pitch, first=0, n=None):
        filled.append((which, first, self.n if n is None else n))
        return plane(self, which, pitch, first, n)
    monkeypatch.setattr(aln.SamBatch, 'plane', counted)
    out = tmp_path / 'out.sam'
    info = recalibrate.recalibrate_bam(fixture['paths'][oq, source], use_oq=use_oq, kmers=dict(k=15), output=str(out))
    assert info['reads'] == 600 and info['k'] == 15
    run = recalibrate.LAST_RUN['aligned']
    n, pitch = 600, 64
    assert run == dict(alignments=n, pitch=pitch, h2d_plane_bytes=n * pitch * len(planes), planes=planes)
    assert len(set(run['planes'])) == len(run['planes'])
    assert sorted(filled) == sorted(({'SEQ': 0, 'QUAL': 1, 'OQ': 2}[p], 0, n) for p in planes)
    assert [w for w, _, _ in filled].count(0) == 1
    assert len(_records(out.read_text())) == n


def test_a_letter_outside_acgtn_still_gives_the_two_commands_bytes(fixture, kbbq, tmp_path):
    """One forward read with an 'R' in its aligned part, among qualities below 6 (the edit of test_gpu_bqsr_kmers.py): the fused
    tally and the 4-bit canonical rows refuse it, the character rows count it -- on the planes that stay for the apply.  On the
    records without OQ tags, whose context `applybqsr` takes from QUAL: with the tag's qualities, all above 5, beside the 'R' the
    second command stops at that record with the reference's TypeError, and so does the one run."""
    lines = fixture['texts']['none'].split('\n')
    idx, hit = 0, None
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
    p = tmp_path / 'weird.sam'
    p.write_text('\n'.join(lines))
    grp = tmp_path / 'two.grp'
    kbbq('bqsr', '-b', p, '--kmers', '-k', '15', '-g', grp)
    want, _ = kbbq('applybqsr', '-b', p, '-g', grp, '-s')
    mine = tmp_path / 'one.grp'
    got, said = kbbq('recalibrate', '-b', p, '--kmers', '-k', '15', '-s', '-g', mine)
    assert 'R' in _records(got)[hit][9] and len(said) == 1
    assert got == want and mine.read_bytes() == grp.read_bytes()
    # ... and with OQ tags: the same error for the same record from either
    tagged = fixture['texts']['all'].split('\n')
    j = [i for i, ln in enumerate(tagged) if ln and not ln.startswith('@')][hit]
    f, g = tagged[j].split('\t'), _records(p.read_text())[hit]
    tagged[j] = '\t'.join(f[:9] + g[9:11] + f[11:])
    q = tmp_path / 'weird_oq.sam'
    q.write_text('\n'.join(tagged))
    kbbq('bqsr', '-b', q, '--kmers', '-k', '15', '-g', tmp_path / 'oq.grp')
    with pytest.raises(TypeError, match='read %d: base outside ACGTN' % hit) as theirs:
        kbbq('applybqsr', '-b', q, '-g', tmp_path / 'oq.grp')
    with pytest.raises(TypeError, match='read %d: base outside ACGTN' % hit) as ours:
        kbbq('recalibrate', '-b', q, '--kmers', '-k', '15')
    assert str(ours.value) == str(theirs.value) and ours.value.read_index == theirs.value.read_index == hit


def test_the_command_as_a_process_imports_no_torch(fixture, tmp_path):
    """`python -m kbbq.main recalibrate -b ... --kmers` on one GPU: device memory from the library's own C ABI, as `bqsr --kmers`."""
    aln = fixture['paths']['half', 'sam']
    grp, want = tmp_path / 'two.grp', tmp_path / 'two.sam'
    for argv in (['bqsr', '-b', aln, '--kmers', '-k', '15', '-g', str(grp)], ['applybqsr', '-b', aln, '-g', str(grp), '-s', '-o', str(want)]):
        r = subprocess.run([sys.executable, '-m', 'kbbq.main'] + argv, capture_output=True, timeout=300, env=ENV)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
    code = ('import sys\nfrom kbbq import main\nmain.main(sys.argv[1:])\nsys.stdout.flush()\n'
            'sys.stderr.write("torch imported: %s\\n" % ("torch" in sys.modules))\n')
    r = subprocess.run([sys.executable, '-c', code, 'recalibrate', '-b', aln, '--kmers', '-k', '15', '-s'], capture_output=True,
                       timeout=300, env=ENV)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert 'torch imported: False' in r.stderr.decode()
    assert r.stdout == want.read_bytes()
    assert len([ln for ln in r.stderr.decode().split('\n') if ln.startswith('kbbq recalibrate: k=15 min_count=')]) == 1


def _port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_a_process_group_is_refused(fixture, tmp_path):
    """A group of one rank (KBBQ_DIST_ALWAYS=1, gloo), joined before the command is called (tests/dist_recalibrate_bam_worker.py):
    ValueError naming the way out, a non-zero exit, no output file, no report."""
    out, grp = tmp_path / 'ranks.sam', tmp_path / 'ranks.grp'
    env = dict(ENV, HSA_ENABLE_IPC_MODE_LEGACY='0', KBBQ_DIST_ALWAYS='1', KBBQ_DIST_BACKEND='gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
           '--master-port', str(_port()), os.path.join(ROOT, 'tests', 'dist_recalibrate_bam_worker.py'),
           fixture['paths']['all', 'sam'], str(out), str(grp)]
    r = subprocess.run(cmd, env=env, capture_output=True, timeout=300)
    stdout, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode != 0
    assert 'group: initialised=True world=1' in stdout, (stdout, err[-3000:])
    assert 'function: recalibrate -b --kmers does not run across ranks' in stdout, (stdout, err[-3000:])
    assert re.search(r'ValueError: recalibrate -b --kmers does not run across ranks', err), err[-3000:]
    assert '`kbbq bqsr -b aln.bam --kmers -g model.grp` on one GPU' in err and '`kbbq applybqsr' in err
    assert not out.exists() and not grp.exists()
