"""--bgzf on the command line, on the MI355X: for `recalibrate -f`, `recalibrate -c`, `correct`, `applybqsr` and `recalibrate -b
--kmers` the output with the option, to -o and to stdout, inflates (gzip.decompress: CRC32 and ISIZE of every block checked)
to the bytes of the run without it, and the `kbbq ...:` lines of stderr are the same; without the option a name ending in .gz
stays plain; under three gloo ranks the rank files are complete BGZF files whose concatenation inflates to the one-process
bytes, also through a shared stdout; `correct` reads a file the option wrote as it reads the plain one."""
import glob
import gzip
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import kmer_bqsr_model as B
import kmer_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = 3
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
HEAD = bytes.fromhex('1f8b08040000000000ff060042430200')


@pytest.fixture
def kbbq(monkeypatch, capfdbinary):
    """The command line in this process: main.main(argv) -> (stdout bytes, its `kbbq ...:` lines of stderr)."""
    from kbbq import main
    monkeypatch.setenv('KBBQ_USE_TORCH', '1')                      # this process has torch tensors already
    monkeypatch.setenv('KBBQ_BGZF_SLAB_BLOCKS', '2')               # several slabs in flight on these small files
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_DIST_ALWAYS'):
        monkeypatch.delenv(var, raising=False)

    def run(*argv):
        capfdbinary.readouterr()
        main.main([str(a) for a in argv])
        sys.stdout.flush()
        sys.stderr.flush()
        out, err = capfdbinary.readouterr()
        assert b'Traceback' not in err
        return out, [ln for ln in err.decode().split('\n') if ln.startswith('kbbq ')]
    return run


@pytest.fixture(scope='module')
def inputs(tmp_path_factory):
    """reads.fq (shortest reads first: `recalibrate -f` takes non-decreasing lengths; about 9 blocks of text) and a SAM file."""
    import oracle_bqsr as OQ
    d = tmp_path_factory.mktemp('bgzf_cli')
    seq, meta = M.synth(9, genome_len=10000, depth=30, err=0.01, len_lo=80, len_hi=200)[:2]
    order = np.argsort(meta, kind='stable')
    seq, meta = seq[order], meta[order].astype(np.int64)
    qual = (np.random.default_rng(3).integers(2, 41, size=seq.shape) + 33).astype(np.uint8)
    fq = d / 'reads.fq'
    fq.write_text(''.join('@SRR77.%d\n%s\n+\n%s\n' % (i, seq[i, :meta[i]].tobytes().decode(), qual[i, :meta[i]].tobytes().decode())
                          for i in range(seq.shape[0])))
    assert fq.stat().st_size > 8 * 65280
    sam = OQ.synth_bqsr_set(str(d), **B.FIXTURE)['sam']
    return dict(dir=d, fq=str(fq), sam=sam)


@pytest.fixture
def made(inputs, kbbq):
    """... with what two of the commands need and the GPU makes: the corrected reads, a report."""
    d = inputs['dir']
    if 'cor' not in inputs:
        kbbq('correct', '-f', inputs['fq'], '-o', d / 'cor.fq')
        kbbq('bqsr', '-b', inputs['sam'], '--kmers', '-k', 15, '-g', d / 'sam.report')
        inputs.update(cor=str(d / 'cor.fq'), report=str(d / 'sam.report'))
    return inputs


def commands(x):
    return dict(recalibrate_f=['recalibrate', '-f', x['fq'], x['cor']],
                recalibrate_c=['recalibrate', '-c', x['fq']],
                correct=['correct', '-f', x['fq']],
                applybqsr=['applybqsr', '-b', x['sam'], '-g', x['report']],
                recalibrate_b=['recalibrate', '-b', x['sam'], '--kmers', '-k', '15'])


def bgzf_blocks(data):
    """The ISIZE of every block of a BGZF file, the headers checked; the file ends with the EOF block."""
    sizes, at = [], 0
    while at < len(data):
        assert data[at:at + 16] == HEAD
        size = int.from_bytes(data[at + 16:at + 18], 'little') + 1
        sizes.append(int.from_bytes(data[at + size - 4:at + size], 'little'))
        at += size
    assert at == len(data) and data[-28:] == EOF
    return sizes


@pytest.mark.parametrize('command', ['recalibrate_f', 'recalibrate_c', 'correct', 'applybqsr', 'recalibrate_b'])
def test_the_output_inflates_to_the_plain_bytes(made, kbbq, tmp_path, command):
    argv = commands(made)[command]
    plain_out, plain_said = kbbq(*argv)
    assert len(plain_out) > 65280
    out, said = kbbq(*argv, '-o', tmp_path / 'plain.gz')            # no suffix detection: plain under a .gz name
    assert out == b'' and said == plain_said and (tmp_path / 'plain.gz').read_bytes() == plain_out
    out, said = kbbq(*argv, '--bgzf', '-o', tmp_path / 'out.gz')
    data = (tmp_path / 'out.gz').read_bytes()
    assert out == b'' and said == plain_said
    assert gzip.decompress(data) == plain_out
    sizes = bgzf_blocks(data)
    whole, rest = divmod(len(plain_out), 65280)
    assert sizes == [65280] * whole + [rest] * (rest > 0) + [0]         # cut every 65280 bytes, then the EOF block
    assert len(data) < len(plain_out) * 0.7
    out, said = kbbq(*argv, '--bgzf')
    assert said == plain_said
    assert out == data                                               # stdout and -o: the same file, a function of the text alone


def test_correct_reads_what_the_option_wrote(made, kbbq, tmp_path):
    kbbq('correct', '-f', made['fq'], '-o', tmp_path / 'out.fq')
    kbbq('correct', '-f', made['fq'], '--bgzf', '-o', tmp_path / 'out.fq.gz')
    assert gzip.decompress((tmp_path / 'out.fq.gz').read_bytes()) == (tmp_path / 'out.fq').read_bytes()
    _, said = kbbq('correct', '-f', tmp_path / 'out.fq', '-o', tmp_path / 'a.fq')
    _, said_gz = kbbq('correct', '-f', tmp_path / 'out.fq.gz', '-o', tmp_path / 'b.fq')
    assert said == said_gz and (tmp_path / 'a.fq').read_bytes() == (tmp_path / 'b.fq').read_bytes()


def test_the_command_as_a_process_imports_no_torch(made, kbbq, tmp_path):
    """`python -m kbbq.main recalibrate -f A B --bgzf` on one GPU: the writer's slabs and device buffers come from the library's
    own C ABI (kbbq/_hipmem.py), and the file is the one the process with torch writes."""
    kbbq('recalibrate', '-f', made['fq'], made['cor'], '--bgzf', '-o', tmp_path / 'torch.gz')
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'), KBBQ_BGZF_SLAB_BLOCKS='2')
    for var in ('RANK', 'WORLD_SIZE', 'KBBQ_USE_TORCH', 'KBBQ_DIST_ALWAYS'):
        env.pop(var, None)
    code = ('import sys\nfrom kbbq import main\nmain.main(sys.argv[1:])\nsys.stdout.flush()\n'
            'sys.stderr.write("torch imported: %s\\n" % ("torch" in sys.modules))\n')
    r = subprocess.run([sys.executable, '-c', code, 'recalibrate', '-f', made['fq'], made['cor'], '--bgzf'], capture_output=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert 'torch imported: False' in r.stderr.decode()
    assert r.stdout == (tmp_path / 'torch.gz').read_bytes()


# ---- ranks ------------------------------------------------------------------------------------------------------------------
def _port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _ranks(argv, timeout=400):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=os.path.join(ROOT, 'kbbq-py_amd'), KBBQ_BGZF_SLAB_BLOCKS='2')
    env.setdefault('KBBQ_DIST_BACKEND', 'gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(RANKS), '--master-addr',
           '127.0.0.1', '--master-port', str(_port()), os.path.join(ROOT, 'tests', 'dist_cli_worker.py')] + [str(a) for a in argv]
    return subprocess.run(cmd, env=env, capture_output=True, timeout=timeout)


def test_rank_files_are_bgzf_files_that_join_to_the_one_process_bytes(made, kbbq, tmp_path):
    want, _ = kbbq('recalibrate', '-f', made['fq'], made['cor'])
    out = str(tmp_path / 'out.fq.gz')
    r = _ranks(['recalibrate', '-f', made['fq'], made['cor'], '--bgzf', '-o', out])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    parts = sorted(glob.glob(out + '.rank*'))
    assert len(parts) == RANKS and r.stdout == b''
    files = [open(p, 'rb').read() for p in parts]
    for data in files:
        assert len(bgzf_blocks(data)) >= 2                           # every rank's file is complete, its own EOF block included
    assert b''.join(gzip.decompress(data) for data in files) == want
    assert gzip.decompress(b''.join(files)) == want                  # joined, then inflated


def test_ranks_share_a_stdout_in_rank_order(made, kbbq):
    want, said = kbbq('correct', '-f', made['fq'])
    r = _ranks(['correct', '-f', made['fq'], '--bgzf'])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert gzip.decompress(r.stdout) == want
    assert r.stdout.count(EOF) >= RANKS                              # a complete file from every rank, one after the other
    assert [ln for ln in r.stderr.decode().split('\n') if ln.startswith('kbbq correct:')] == said
