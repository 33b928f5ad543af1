"""
`--bam-out`: the alignments `applybqsr` and `recalibrate -b --kmers` write, as a BAM file whose records are assembled and
deflated on the GPU (include/kbbq_hip.h "BAM output", csrc/kbbq_bam_out.h, csrc/sam_host.cpp).

The uncompressed stream is defined by the SAM text the same command writes without the option (SAM specification 4.2; the
tests' bamwriter.sam_to_bam_bytes of that text).  The work is divided: the host writes, in parallel over records, what only
the text knows -- a compact skeleton of fixed fields, QNAME, CIGAR and encoded tags, and a descriptor per record -- and only
those go up; the device adds SEQ, packed from the character plane the apply kernel read, and QUAL, from the plane it wrote, at
every record's offset of the stream (kbbq_bam_assemble_dev), so neither plane crosses the bus again.

BamWriter(raw) owns the device stream buffer, the carry and the binary sink.  The stream is cut every BLOCK = 65280 bytes
whatever the record and slab boundaries are: after a slab is assembled behind the carry, the whole blocks are deflated where
they lie (kbbq_bgzf_deflate_dev, KBBQ_BGZF_SLAB_BLOCKS blocks a call) and only compressed bytes come back, through a
page-locked buffer as in kbbq/_bgzf.py; what is left below a block is copied, device to device, to the front of the buffer and
waits for the next slab; close() deflates it and writes the 28-byte EOF block.  The file is a function of the stream alone.
A new quality below 0 fits SAM text but not BAM: the assemble kernel leaves the lowest such row in a word that is read after
every slab, before any byte of the slab reaches the sink -- ValueError with .read_index.

h2d_bytes (header, skeletons, descriptors), d2h_bytes (compressed blocks), stream_bytes and file_bytes count what moved, as
BgzfWriter counts text_bytes / file_bytes.  deflate=: a function text -> BGZF blocks in the place of the GPU; the planes are then
NumPy arrays and the records are assembled by the host twin (kbbq_bam_assemble) -- the tests' stand-in.

records() has a second way to its descriptors and skeleton: a batch whose records are resident as BAM records (kbbq/_bamin.py
DeviceBatch.stream, KBBQ_GPU_BAM=1) has them made on the device by kbbq_bam_recode_dev (include/kbbq_hip.h "BAM recode"); only the
keep mask goes up, and everything behind that point -- assemble, the quality error, the index, the drain -- is the same.  close()
frees the resident stream.

index= (--bam-index: 'auto', 'bai' or 'csi'; kbbq/_bamindex.py, include/kbbq_hip.h "BAM index"): the file's index, made in the
same pass.  header() decides the format and lays the file-long linear array out on the device; after a slab is assembled the
index kernels (kbbq_bam_index_dev; kbbq_bam_index with deflate=) read the same skeleton and descriptors and send back one
32-byte run per (refID, bin) run of the slab; the compressed sizes of the blocks are read off the packed bytes on their way to
the sink; close() downloads the linear array, serialises (a CSI through the same deflate call) and leaves the bytes in
index_data -- with index_path, in index_path + '.bai' / '.csi'.  index_bytes, index_runs, index_d2h_bytes count it.  Without
index= nothing of this is touched or launched.
"""
import ctypes
import io

import numpy as np

from ._bgzf import BLOCK, EOF, slab_blocks


class _HostEngine:
    """Plain memory, kbbq_bam_assemble and a function text -> BGZF blocks."""

    def __init__(self, deflate):
        self.fn = deflate

    def buffer(self, nbytes):
        return np.empty(int(nbytes), dtype=np.uint8)

    def staging(self, nbytes):
        return np.empty(int(nbytes), dtype=np.uint8)

    def upload(self, stage, nbytes):
        return stage

    def put(self, buf, at, data):
        buf[at:at + len(data)] = data

    def move(self, dst, src, lo, n):
        dst[:n] = src[lo:lo + n].copy()

    def assemble(self, d_stage, desc_bytes, skel_bytes, n, seq, qplane, pitch, buf, carry):
        from . import _native as N
        bad = ctypes.c_int64(-1)
        N.check(N.load().kbbq_bam_assemble(N.ptr(d_stage[desc_bytes:]), skel_bytes, N.ptr(d_stage), n, N.ptr(seq), N.ptr(qplane), pitch,
                                           N.ptr(buf), carry, buf.nbytes, ctypes.byref(bad)))
        return int(bad.value)

    def deflate(self, buf, lo, n):
        return self.fn(memoryview(buf)[lo:lo + n])

    # ---- index=: the linear array in plain memory, kbbq_bam_index
    def index_open(self, lin_off):
        self.lin_off = np.ascontiguousarray(lin_off, dtype=np.uint64)
        self.linear = np.full(max(int(lin_off[-1]), 1), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)

    def index_slab(self, d_stage, desc_bytes, skel_bytes, n, base, depth):
        from . import _native as N
        runs = np.empty(n * N.BAM_RUN_BYTES, dtype=np.uint8)
        count, bad = ctypes.c_int64(0), ctypes.c_int64(-1)
        N.check(N.load().kbbq_bam_index(N.ptr(d_stage[desc_bytes:]), skel_bytes, N.ptr(d_stage), n, base, depth, N.ptr(self.lin_off),
                                        len(self.lin_off) - 1, N.ptr(self.linear), N.ptr(runs), n, ctypes.byref(count), ctypes.byref(bad)))
        return runs[:count.value * N.BAM_RUN_BYTES], 0

    def index_linear(self):
        return self.linear[:int(self.lin_off[-1])], 0

    def pack(self, data):
        return bytes(self.fn(memoryview(data))) if len(data) else b''

    def close(self):
        pass


class _GpuEngine:
    """Device memory of the backend the process uses (kbbq/_device.py), kbbq_bam_assemble_dev and kbbq_bgzf_deflate_dev."""

    def __init__(self):
        from . import _device as dev
        self.dev, self.t = dev, dev._torch()
        self.device = self.t.cuda.current_device()
        self.piece = slab_blocks() * BLOCK
        self.scratch = self.d_stage = self.d_lin_off = self.d_linear = None

    def buffer(self, nbytes):
        return self.t.empty(int(nbytes), dtype=self.t.uint8, device='cuda')

    def staging(self, nbytes):
        return self.dev.pinned('bamout', 'stage', int(nbytes)).numpy()

    def upload(self, stage, nbytes):
        pin = self.dev.pinned('bamout', 'stage', nbytes)
        if self.d_stage is None or self.d_stage.shape[0] < nbytes:
            self.d_stage = None
            self.d_stage = self.buffer(nbytes + nbytes // 8)
        self.d_stage[:nbytes].copy_(pin[:nbytes], non_blocking=True)
        return self.d_stage

    def put(self, buf, at, data):
        buf[at:at + len(data)].copy_(self.t.from_numpy(np.ascontiguousarray(data)))

    def move(self, dst, src, lo, n):
        dst[:n].copy_(src[lo:lo + n])

    def assemble(self, d_stage, desc_bytes, skel_bytes, n, seq, qplane, pitch, buf, carry):
        N = self.dev.N
        ctx = self.dev.context(self.device)
        bad = ctypes.c_int64(-1)
        N.check(N.load().kbbq_bam_assemble_dev(ctx.handle, N.ptr(d_stage.data_ptr() + desc_bytes), skel_bytes, N.ptr(d_stage), n,
                                               N.ptr(seq), N.ptr(qplane), pitch, N.ptr(buf), carry, buf.shape[0], ctypes.byref(bad)))
        return int(bad.value)

    def recode(self, stream, first, n, set_oq, keep, desc_bytes):
        """The descriptors and the skeleton of records [first, first + n) of a resident record stream (kbbq/_bamin.py Stream), made
        where they are read (kbbq_bam_recode_dev): (the device buffer: descriptors | skeleton, skeleton bytes, stream bytes, bytes
        that went up)."""
        from . import _bamin
        cap = stream.skel_cap(first, n, set_oq)
        nbytes = desc_bytes + cap
        if self.d_stage is None or self.d_stage.shape[0] < nbytes:
            self.d_stage = None
            self.d_stage = self.buffer(nbytes + nbytes // 8)
        d_keep = None if keep is None else self.t.from_numpy(keep).cuda()
        skel_bytes, stream_bytes, status = _bamin.recode_device(stream, first, n, set_oq, d_keep, self.d_stage, desc_bytes, cap)
        if status:
            raise RuntimeError('kbbq_bam_recode_dev: status 0x%x for records the open vouched for' % status)
        return self.d_stage, skel_bytes, stream_bytes, 0 if keep is None else keep.nbytes

    def deflate(self, buf, lo, n):
        N, t = self.dev.N, self.t
        ctx = self.dev.context(self.device)
        lib = N.load()
        if self.scratch is None:
            blocks = self.piece // BLOCK
            bound = int(lib.kbbq_bgzf_bound(self.piece, BLOCK))
            self.scratch = (self.buffer(blocks * N.BGZF_SLOT), self.buffer(4 * blocks), self.buffer(bound),
                            self.dev.pinned('bamout', 'out', bound))
        d_blocks, d_sizes, d_packed, out = self.scratch
        total = ctypes.c_size_t(0)
        N.check(lib.kbbq_bgzf_deflate_dev(ctx.handle, N.ptr(buf.data_ptr() + lo), n, BLOCK, N.ptr(d_blocks), N.ptr(d_sizes),
                                          N.ptr(d_packed), ctypes.byref(total)))
        out[:total.value].copy_(d_packed[:total.value])
        return memoryview(out.numpy())[:total.value]

    # ---- index=: the linear array and the references' window offsets in device memory, kbbq_bam_index_dev
    def index_open(self, lin_off):
        self.n_ref, self.windows = len(lin_off) - 1, int(lin_off[-1])
        self.d_lin_off = self.buffer(8 * len(lin_off))
        self.put(self.d_lin_off, 0, np.ascontiguousarray(lin_off, dtype=np.uint64).view(np.uint8))
        self.d_linear = self.buffer(8 * max(self.windows, 1))
        self.put(self.d_linear, 0, np.full(8 * max(self.windows, 1), 0xFF, dtype=np.uint8))

    def index_slab(self, d_stage, desc_bytes, skel_bytes, n, base, depth):
        N = self.dev.N
        ctx = self.dev.context(self.device)
        runs = np.empty(n * N.BAM_RUN_BYTES, dtype=np.uint8)
        count, bad = ctypes.c_int64(0), ctypes.c_int64(-1)
        N.check(N.load().kbbq_bam_index_dev(ctx.handle, N.ptr(d_stage.data_ptr() + desc_bytes), skel_bytes, N.ptr(d_stage), n, base,
                                            depth, N.ptr(self.d_lin_off), self.n_ref, N.ptr(self.d_linear), N.ptr(runs), n,
                                            ctypes.byref(count), ctypes.byref(bad)))
        return runs[:count.value * N.BAM_RUN_BYTES], count.value * N.BAM_RUN_BYTES + 24     # the runs, four words, the window total

    def index_linear(self):
        return self.d_linear.cpu().numpy().view(np.uint64)[:self.windows].copy(), 8 * self.windows

    def pack(self, data):
        out = []
        for lo in range(0, len(data), self.piece):
            part = np.frombuffer(data, dtype=np.uint8, count=min(self.piece, len(data) - lo), offset=lo).copy()
            d_text = self.buffer((len(part) + 15) // 16 * 16)
            self.put(d_text, 0, part)
            out.append(bytes(self.deflate(d_text, 0, len(part))))
        return b''.join(out)

    def close(self):
        self.scratch = self.d_stage = self.d_lin_off = self.d_linear = None
        self.dev.release_pinned('bamout')


class BamWriter:
    """header(bam), records(...) slab by slab, close() over the binary sink `raw` (see the module's text).  A context manager:
    leaving it on an exception closes the sink without the carry and without the EOF block.  close_raw: close() closes `raw` too."""

    def __init__(self, raw, close_raw=False, deflate=None, index=None, index_path=None):
        if raw is None or isinstance(raw, io.TextIOBase) or not hasattr(raw, 'write'):
            raise ValueError('--bam-out writes bytes: the sink must be a binary file (a text-only stdout cannot take it)')
        self._raw, self._close_raw = raw, close_raw
        self._engine = _HostEngine(deflate) if deflate is not None else _GpuEngine()
        self._piece = slab_blocks() * BLOCK
        self._buf, self._carry = None, 0
        self.closed = False
        self.h2d_bytes = self.d2h_bytes = self.stream_bytes = self.file_bytes = 0
        # index= ('auto', 'bai', 'csi'): header() decides the format; close() leaves the file's bytes in index_data and, with
        # index_path, writes them to index_path + '.bai' / '.csi'
        self._index_kind, self._index_path, self._index = index, index_path, None
        self.index_format = self.index_data = None
        self.index_bytes = self.index_runs = self.index_d2h_bytes = 0
        self._resident = None                 # a DeviceBatch whose record stream fed records(): released by close()

    def __enter__(self):
        return self

    def __exit__(self, kind, exc, tb):
        if kind is None:
            self.close()
        else:
            self._finish()

    # ---- the stream buffer: [carry | the slab being assembled]
    def _room(self, need):
        """A buffer of at least `need` bytes with the carry at its front."""
        if self._buf is not None and self._buf.shape[0] >= need:
            return
        new = self._engine.buffer((need + need // 8 + 15) // 16 * 16)
        if self._carry:
            self._engine.move(new, self._buf, 0, self._carry)
        self._buf = new

    def _drain(self, total, last=False):
        """Bytes [0, total) of the buffer: the whole blocks (last: all of it) deflated and written, the rest carried."""
        whole = total if last else total // BLOCK * BLOCK
        for lo in range(0, whole, self._piece):
            packed = self._engine.deflate(self._buf, lo, min(self._piece, whole - lo))
            self._raw.write(packed)
            if self._index is not None:
                self._index.blocks(packed)
            self.d2h_bytes += len(packed)
            self.file_bytes += len(packed)
        if whole and total > whole:
            self._engine.move(self._buf, self._buf, whole, total - whole)
        self._carry = total - whole

    def _open(self):
        if self.closed:
            raise ValueError('write to a closed BamWriter')

    # ---- the file
    def header(self, bam):
        """The stream's head of an aln.AlignmentFile: magic, the header text as read, the references of its @SQ lines."""
        from . import _native as N
        self._open()
        lib, native = N.load(), getattr(bam.batch(), '_native', None)
        need = ctypes.c_size_t(0)
        if native is None:
            # a DeviceBatch (kbbq/_bamin.py): the scan's header lines through the same code (kbbq_bam_header_text)
            text = np.frombuffer(''.join(line + '\n' for line in bam.header).encode('latin-1'), dtype=np.uint8)
            call = lambda out, cap: lib.kbbq_bam_header_text(N.ptr(text) if text.nbytes else None, text.nbytes, out, cap, ctypes.byref(need))   # noqa: E731
        else:
            call = lambda out, cap: lib.kbbq_bam_header(native, out, cap, ctypes.byref(need))   # noqa: E731
        N.check(call(None, 0))
        head = np.empty(need.value, dtype=np.uint8)
        N.check(call(N.ptr(head), head.nbytes))
        if self._index_kind is not None:
            from . import _bamindex
            if self._index is not None or self.stream_bytes:
                raise ValueError('index=: the header is written once, before the records')
            self.index_format, depth = _bamindex.resolve(self._index_kind, bam.header)
            self._index = _bamindex.Index(self.index_format, depth, [ln for _, ln, _ in _bamindex.references(bam.header)])
            self._engine.index_open(self._index.lin_off)
        self._room(self._carry + head.nbytes)
        self._engine.put(self._buf, self._carry, head)
        self.h2d_bytes += head.nbytes
        self.stream_bytes += head.nbytes
        self._drain(self._carry + head.nbytes)

    def records(self, batch, first, n, set_oq, keep_qual, seq, qplane, pitch):
        """Alignments [first, first + n) of the reader's batch.  seq, qplane: their rows of the SEQ character plane and of the
        apply's output plane, [n, pitch], where the engine works (device tensors; NumPy arrays with deflate=); keep_qual: a
        bool array, true for a record whose QUAL stays as read (a '*' QUAL always does).  ValueError with .read_index for a new
        quality below 0, before any byte of these records reaches the sink."""
        from . import _native as N
        self._open()
        if n <= 0:
            return
        lib = N.load()
        keep = None if keep_qual is None else np.ascontiguousarray(keep_qual, dtype=np.uint8)
        skel_bytes, stream_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
        desc_bytes = (4 * N.BAM_DESC_WORDS * n + 15) // 16 * 16
        if getattr(batch, 'stream', None) is not None:
            # the second way: the records are resident as BAM records, descriptors and skeleton are made on the device from them
            self._resident = batch
            d_stage, skel_bytes.value, stream_bytes.value, up = self._engine.recode(batch.stream, first, n, set_oq, keep, desc_bytes)
            self.h2d_bytes += up
        else:
            desc = np.empty((n, N.BAM_DESC_WORDS), dtype=np.uint32)
            N.check(lib.kbbq_bam_layout(batch._native, first, n, int(bool(set_oq)), N.ptr(keep), N.ptr(desc), ctypes.byref(skel_bytes),
                                        ctypes.byref(stream_bytes)))
            nbytes = desc_bytes + skel_bytes.value
            stage = self._engine.staging(nbytes)
            stage[:desc.nbytes] = desc.reshape(-1).view(np.uint8)
            N.check(lib.kbbq_bam_skeleton(batch._native, first, n, int(bool(set_oq)), N.ptr(desc), N.ptr(stage[desc_bytes:]), skel_bytes.value))
            d_stage = self._engine.upload(stage, nbytes)
            self.h2d_bytes += nbytes
        total = self._carry + stream_bytes.value
        self._room(total)
        bad = self._engine.assemble(d_stage, desc_bytes, skel_bytes.value, n, seq, qplane, pitch, self._buf, self._carry)
        if bad >= 0:
            exc = ValueError('alignment %d: a new quality below 0 cannot be written as BAM (SAM text holds it: without --bam-out)'
                             % (first + bad))
            exc.read_index = first + bad
            raise exc
        if self._index_kind is not None:
            if self._index is None:
                raise ValueError('index=: records before the header (the index needs the @SQ lines)')
            runs, back = self._engine.index_slab(d_stage, desc_bytes, skel_bytes.value, n, self.stream_bytes, self._index.depth)
            self._index.runs(runs.view(self._index_run_dtype()))
            self.index_d2h_bytes += back
        self.stream_bytes += stream_bytes.value
        self._drain(total)

    @staticmethod
    def _index_run_dtype():
        from . import _bamindex
        return _bamindex.RUN

    def _write_index(self):
        """Before the EOF block is written: file_bytes is its offset."""
        from . import _bamindex
        linear, back = self._engine.index_linear()
        self.index_d2h_bytes += back
        data = self._index.data(linear, self.file_bytes)
        if self.index_format == 'csi':
            data = self._engine.pack(data) + EOF
        self.index_data, self.index_bytes, self.index_runs = data, len(data), self._index.n_runs
        if self._index_path is not None:
            with open(_bamindex.index_path(self._index_path, self.index_format), 'wb') as fh:
                fh.write(data)

    def _finish(self):
        self.closed = True
        self._buf = None
        if self._resident is not None:
            self._resident.release_stream()
            self._resident = None
        self._engine.close()
        if self._close_raw:
            self._raw.close()

    def close(self):
        if self.closed:
            return
        try:
            if self._carry:
                self._drain(self._carry, last=True)
            if self._index is not None:
                self._write_index()
            self._raw.write(EOF)
            self.file_bytes += len(EOF)
            self._raw.flush()
        finally:
            self._finish()


def check(bam, lo=0, hi=None):
    """What BAM cannot hold of alignments [lo, hi) of an aln.AlignmentFile (kbbq_bam_check): ValueError naming the first such
    alignment, with .read_index -- to be called before the output file is created."""
    from . import _native as N
    if getattr(bam.batch(), 'stream', None) is not None:
        return                                # BAM records the recode vouched for (kbbq/_bamin.py open_device): BAM holds them
    hi = len(bam) if hi is None else hi
    bad = ctypes.c_int64(-1)
    try:
        N.check(N.load().kbbq_bam_check(bam.batch()._native, lo, hi - lo, ctypes.byref(bad)))
    except ValueError as exc:
        if bad.value >= 0:
            exc.read_index = int(bad.value)
        raise


def open_sink(path, index=None):
    """A BamWriter over the binary file `path`; index: its index beside it (path + '.bai' / '.csi')."""
    raw = open(path, 'wb')
    try:
        return BamWriter(raw, close_raw=True) if index is None else BamWriter(raw, close_raw=True, index=index, index_path=path)
    except BaseException:
        raw.close()
        raise


def stdout_sink():
    """A BamWriter over the process's binary stdout (stdout itself stays open)."""
    import sys
    sys.stdout.flush()
    return BamWriter(getattr(sys.stdout, 'buffer', None))
