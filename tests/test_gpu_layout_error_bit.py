"""
GPU tests (-m gpu) of KBBQ_ROWS_ERRBIT in the layouts and the file path: the C++ packer without a corrected plane
(`laid_from_reader(keep_corrected=False)`) against the layout pass on the same reads, the entry points that refuse the
flag on a live context, and `recalibrate -f A B` -- resident and streamed -- against the recorded output of the golden
cases (what the file path wrote before the flag existed).
"""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import dev, _files              # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n,S,nrg,single_end', [(6000, 150, 1, False), (6000, 150, 4, False), (5001, 150, 1, True), (4000, 100, 3, True)])
def test_the_packer_without_a_corrected_plane(dev, tmp_path, n, S, nrg, single_end):
    from kbbq import fastx
    from test_packer_layouts import _pair_files
    rng = np.random.default_rng(n + S)
    fa, fb = _pair_files(tmp_path, rng, n, S, nrg, single_end)
    infer = nrg > 1
    A, B, info = fastx.PairScan(fa, fb, infer).result()
    R = info[2]
    pitch = fastx.pitch_for(S)
    rows = dev.ReadBatch.from_reader(A, B, infer, 0, n, pitch)
    want = dev.lay_out(rows, R, S, packed=True)
    assert want.errbit and want.nib and isinstance(want, dev.PairBatch) and want.cseq is not None
    kept = dev.laid_from_reader(A, B, infer, 0, n, pitch, R, packed=True)
    for slab in (1 << 17, 998):
        got = dev.laid_from_reader(A, B, infer, 0, n, pitch, R, packed=True, slab=slab, keep_corrected=False)
        assert got.errbit and got.cseq is None and got.n == want.n and got.twins == want.twins == single_end
        for name in ('seq', 'qual', 'meta'):
            assert np.array_equal(getattr(got, name)[:want.n].cpu().numpy(), getattr(want, name)[:want.n].cpu().numpy()), (name, slab)
        assert got.h2d_bytes == kept.h2d_bytes - want.n * (want.pitch // 2)          # the corrected plane never crosses PCIe
    # the layout pass itself without a destination for the corrected plane, and both without the flag
    lone = dev.lay_out(rows, R, S, packed=True, keep_corrected=False)
    assert lone.cseq is None and np.array_equal(lone.seq.cpu().numpy(), want.seq.cpu().numpy())
    plain = dev.lay_out(rows, R, S, packed=True, errbit=False)
    got = dev.laid_from_reader(A, B, infer, 0, n, pitch, R, packed=True, errbit=False, keep_corrected=False)
    assert not plain.errbit and not got.errbit and got.cseq is not None           # two planes: K1 needs the second one
    for name in ('seq', 'cseq', 'qual', 'meta'):
        assert np.array_equal(getattr(got, name)[:want.n].cpu().numpy(), getattr(plain, name)[:want.n].cpu().numpy()), name
    assert not int((plain.seq & 0x88).ne(0).sum()) and int((want.seq & 0x88).ne(0).sum())
    # the tally of all of them is one tally
    tabs = []
    for b in (want, lone, plain):
        t = dev.Tables(R, 2 * S)
        dev.accumulate(b, t)
        tabs.append(t.buf.cpu().numpy())
    assert np.array_equal(tabs[0], tabs[1]) and np.array_equal(tabs[0], tabs[2]) and tabs[0].sum() > 0
    assert not [k for k in dev._pinned if k[0] == 'ingest']


def test_entry_points_that_refuse_the_flag(dev):
    """KBBQ_E_ARG (ValueError) naming the call, before anything is launched: the k-mer calls on rows through their Python
    wrappers, K6's 4-bit output, and K1 / K2 / the layout pass on rows the flag does not describe."""
    from kbbq import kmer
    N = dev.N
    S, n = 150, 256
    b = dev.ReadBatch.synthetic(0, n, n, seed=5, len_lo=S, len_hi=S)
    eb = dev.lay_out(b, 1, S, packed=True)
    assert eb.errbit
    with pytest.raises(ValueError, match='kbbq_kmer_count_rows_dev.*KBBQ_ROWS_ERRBIT'):
        kmer.count_batch(eb, k=31, slots=1 << 16)
    with pytest.raises(ValueError, match='KBBQ_ROWS_ERRBIT'):
        kmer.prefilter_batch(eb, 31)
    with pytest.raises(ValueError, match='KBBQ_ROWS_ERRBIT'):
        kmer.gate_batch(eb, 31, 10)
    lib, ctx = N.load(), dev.context()
    t = dev.Tables(1, 2 * S)
    args = lambda batch, flags, pitch: (ctx.handle, N.ptr(batch.seq), None, N.ptr(batch.qual), N.ptr(batch.meta), batch.n, pitch, flags,
                                        1, 2 * S, 0, 0, 6, 6, None, N.ptr(t.buf))
    for flags in (N.ROWS_ERRBIT, N.ROWS_ERRBIT | N.ROWS_PAIRS, N.ROWS_ERRBIT | N.ROWS_NIBBLES):
        assert lib.kbbq_accumulate_rows_dev(*args(eb, flags, eb.pitch)) == N.KBBQ_E_ARG
        assert 'kbbq_accumulate_rows_dev' in lib.kbbq_last_error().decode()
    S50 = dev.lay_out(dev.ReadBatch.synthetic(0, n, n, seed=5, len_lo=50, len_hi=50), 1, 50, packed=True)
    assert isinstance(S50, dev.PairBatch) and S50.nib and not S50.errbit and S50.pitch == 112          # 7 chunks: no instance
    t50 = dev.Tables(1, 100)
    rc = lib.kbbq_accumulate_rows_dev(ctx.handle, N.ptr(S50.seq), None, N.ptr(S50.qual), N.ptr(S50.meta), S50.n, 112,
                                      N.ROWS_PAIRS | N.ROWS_NIBBLES | N.ROWS_ERRBIT, 1, 100, 0, 0, 6, 6, None, N.ptr(t50.buf))
    assert rc == N.KBBQ_E_ARG and 'KBBQ_ROWS_ERRBIT' in lib.kbbq_last_error().decode()
    with pytest.raises(ValueError):
        dev.lay_out(dev.ReadBatch.synthetic(0, n, n, seed=5, len_lo=50, len_hi=50), 1, 50, packed=True, errbit=True)
    # K6's rows are one read to a row: the flag is refused before any other argument is looked at
    rc = lib.kbbq_canonical_reads_rows_dev(ctx.handle, None, None, None, None, None, None, None, None, 0, 160, 150, 6, 6,
                                           N.ROWS_NIBBLES | N.ROWS_ERRBIT, None, None, None, None)
    msg = lib.kbbq_last_error().decode()
    assert rc == N.KBBQ_E_ARG and 'kbbq_canonical_reads_rows_dev' in msg and 'KBBQ_ROWS_ERRBIT' in msg
    ctx.status()
    assert not int(t.buf.sum()) and not int(t50.buf.sum())


@pytest.mark.parametrize('case', ['c1_10k_1rg', 'c3cut_2k_8rg'])
def test_the_file_path_writes_the_recorded_bytes(dev, oracle, tmp_path, case, monkeypatch):
    from kbbq import recalibrate
    info, _ = load_golden(case)
    fa, fb = _files(oracle, info, tmp_path)
    out = str(tmp_path / 'out.fq')
    for env in ({}, {'KBBQ_DEVICE_BUDGET': '1M'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        recalibrate.recalibrate_fastq([fa, fb], infer_rg=info['case']['infer_rg'], output=out)
        assert oracle.sha256(open(out, 'rb').read()) == info['output_sha256'], env
        if not env:
            band = recalibrate.LAST_RUN['bands'][0]
            assert 'error bit' in band['layout'] and 'kbbq_fastq_fill_rows' in band['written_by']
