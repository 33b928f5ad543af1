"""
`--bgzf`: the text the commands write -- FASTQ records, SAM lines -- as a BGZF file, deflated on the GPU.

BGZF is gzip made of independent members of at most 64 KiB of text: `zcat`, Python's gzip, this package's own readers and every
downstream tool read it, files joined end to end are a valid file (the rank files of a launcher, joined and then inflated, are
the one-process bytes), and a member is one workgroup's work (csrc/kbbq_bgzf.h, include/kbbq_hip.h "BGZF output").

BgzfWriter(raw) is a binary file-like object over a binary sink.  Whatever the sizes of the write() calls, the stream is cut
every BLOCK = 65280 bytes: the file is a function of the text alone.  The bytes collect in a page-locked slab of SLAB_BLOCKS
blocks; a full slab goes to a worker thread, which uploads it, runs the kernels on the context's stream
(kbbq_bgzf_deflate_dev), downloads the packed blocks -- only compressed bytes come back -- and writes them to the sink while the
caller fills the other slab: two slabs in flight.  close() sends what is left, then the 28-byte EOF block.  flush() waits for the
full slabs that are on their way and flushes the sink; it does not cut a block short, which would make the file depend on
where the flushes fell.  There is no fileno(): the writer is not a file descriptor, and _egress._Reserve stays out of its way.

The commands reach it through `option` and the two sinks below: a public entry point decorated with `option` takes the keyword
`bgzf`, and while it runs with bgzf=True every sink opened by open_sink / stdout_sink / write_text is compressed.  Without the
keyword the sinks are the files they were.  Device memory and page-locked buffers come from the backend the process uses
(kbbq/_device.py: torch, or kbbq/_hipmem.py on the one-GPU command line, which still imports no torch).
"""
import contextlib
import functools
import io
import os
import queue
import sys
import threading

import numpy as np

BLOCK = 65280                          # KBBQ_BGZF_BLOCK_MAX: text bytes of a block
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')      # kbbq_bgzf_eof


def slab_blocks():
    """Blocks of a slab: KBBQ_BGZF_SLAB_BLOCKS, default 256 (16 MiB of text)."""
    return max(1, int(os.environ.get('KBBQ_BGZF_SLAB_BLOCKS') or 256))


class _GpuDeflate:
    """Two page-locked slabs and the native call on them.  slab(i): slab i as a NumPy array; deflate(i, n): the BGZF blocks of
    its first n bytes, valid until the next call.  The device is first touched by the first deflate, on the worker's thread."""

    def __init__(self, nbytes):
        from . import _device as dev
        self.dev, self.nbytes = dev, nbytes
        self.backend = dev._torch()
        self.device = self.backend.cuda.current_device()      # a new thread starts on device 0
        self.pins = {}
        self.buffers = None

    def slab(self, i):
        if i not in self.pins:
            self.pins[i] = self.dev.pinned('bgzf', i, self.nbytes)
        return self.pins[i].numpy()

    def deflate(self, i, n):
        import ctypes
        dev, N, t = self.dev, self.dev.N, self.backend
        with t.cuda.device(self.device):
            ctx = dev.context(self.device)
            lib = N.load()
            if self.buffers is None:
                blocks = (self.nbytes + BLOCK - 1) // BLOCK
                bound = int(lib.kbbq_bgzf_bound(self.nbytes, BLOCK))
                new = lambda nbytes: t.empty(int(nbytes), dtype=t.uint8, device='cuda')     # noqa: E731
                self.buffers = (new(self.nbytes), new(blocks * N.BGZF_SLOT), new(4 * blocks), new(bound),
                                dev.pinned('bgzf', 'out', bound))
            d_text, d_blocks, d_sizes, d_packed, out = self.buffers
            d_text[:n].copy_(self.pins[i][:n], non_blocking=True)
            total = ctypes.c_size_t(0)
            N.check(lib.kbbq_bgzf_deflate_dev(ctx.handle, N.ptr(d_text), n, BLOCK, N.ptr(d_blocks), N.ptr(d_sizes), N.ptr(d_packed),
                                              ctypes.byref(total)))
            out[:total.value].copy_(d_packed[:total.value])
            return memoryview(out.numpy())[:total.value]

    def close(self):
        self.buffers = None
        self.pins = {}
        self.dev.release_pinned('bgzf')


class _CallDeflate:
    """The same over plain memory and a function text -> BGZF blocks (the tests' stand-in for the native call)."""

    def __init__(self, fn, nbytes):
        self.fn, self.slabs = fn, [np.empty(nbytes, dtype=np.uint8) for _ in range(2)]

    def slab(self, i):
        return self.slabs[i]

    def deflate(self, i, n):
        return self.fn(memoryview(self.slabs[i])[:n])

    def close(self):
        pass


class BgzfWriter(io.RawIOBase):
    """write / flush / close over the binary sink `raw` (see the module's text).  close_raw: close() closes `raw` too.
    deflate: a function (text bytes, cut at multiples of BLOCK by the callee) -> BGZF blocks, in the place of the GPU."""

    def __init__(self, raw, close_raw=False, deflate=None):
        super().__init__()
        self._engine = None
        if raw is None or isinstance(raw, io.TextIOBase) or not hasattr(raw, 'write'):
            raise ValueError('--bgzf writes bytes: the sink must be a binary file (a text-only stdout cannot take it)')
        self._raw, self._close_raw = raw, close_raw
        nbytes = slab_blocks() * BLOCK
        self._engine = _CallDeflate(deflate, nbytes) if deflate is not None else _GpuDeflate(nbytes)
        self._nbytes = nbytes
        self._free, self._jobs = queue.Queue(), queue.Queue()
        for i in range(2):
            self._free.put(i)
        self._cur, self._fill, self._buf = None, 0, None
        self._error = None
        self._worker = None
        self.text_bytes = self.file_bytes = 0

    # ---- the worker: slab -> blocks -> sink
    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            i, n = job
            try:
                if self._error is None:
                    packed = self._engine.deflate(i, n)
                    self._raw.write(packed)
                    self.file_bytes += len(packed)
            except BaseException as exc:         # noqa: BLE001 -- raised again by the caller's next write / flush / close
                self._error = exc
            finally:
                self._free.put(i)

    def _submit(self):
        if self._worker is None:
            self._worker = threading.Thread(target=self._run, name='kbbq-bgzf', daemon=True)
            self._worker.start()
        self._jobs.put((self._cur, self._fill))
        self._cur, self._fill, self._buf = None, 0, None

    def _check(self):
        if self._error is not None:
            exc, self._error = self._error, None
            raise exc

    def _drain(self):
        """Wait until both slabs are free again."""
        held = [self._free.get() for _ in range(2 if self._cur is None else 1)]
        for i in held:
            self._free.put(i)

    # ---- the file
    def writable(self):
        return True

    def fileno(self):
        raise io.UnsupportedOperation('a BgzfWriter is not a file descriptor')

    def write(self, data):
        if self.closed:
            raise ValueError('write to a closed BgzfWriter')
        self._check()
        view = memoryview(data).cast('B')
        src, at, n = np.frombuffer(view, dtype=np.uint8), 0, len(view)
        while at < n:
            if self._cur is None:
                self._cur = self._free.get()
                self._buf = self._engine.slab(self._cur)
            m = min(n - at, self._nbytes - self._fill)
            self._buf[self._fill:self._fill + m] = src[at:at + m]
            self._fill += m
            at += m
            if self._fill == self._nbytes:
                self._submit()
        self.text_bytes += n
        return n

    def flush(self):
        if self.closed or getattr(self, '_worker', None) is None:
            return
        self._drain()
        self._check()
        self._raw.flush()

    def close(self):
        if self.closed:
            return
        if self._engine is None:                 # the constructor refused the sink
            super().close()
            return
        try:
            if self._fill:
                self._submit()
            if self._worker is not None:
                self._jobs.put(None)
                self._worker.join()
            self._check()
            self._raw.write(EOF)
            self.file_bytes += len(EOF)
            self._raw.flush()
        finally:
            self._engine.close()
            super().close()
            if self._close_raw:
                self._raw.close()


# ---- the other direction ---------------------------------------------------------------------------------------------------
def inflate(data, stats=None):
    """The text of the BGZF stream `data` (bytes-like), inflated on the GPU (csrc/kbbq_bgzf_inflate.h: a member per workgroup;
    members the kernel does not verify are inflated again on the host).  stats: a dict that receives device_blocks, host_blocks,
    bytes_up, bytes_down.  ValueError for a stream that is not BGZF or is damaged, with the readers' text."""
    import ctypes
    from . import _device as dev
    N = dev.N
    lib = N.load()
    src = np.frombuffer(memoryview(data).cast('B'), dtype=np.uint8)
    nb, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.kbbq_inflate_index(N.ptr(src) if len(src) else None, len(src), None, 0, ctypes.byref(nb), ctypes.byref(total))
    if rc == N.INFLATE_NOT_BGZF:
        raise ValueError('not a BGZF stream')
    N.check(rc)
    out = np.empty(total.value, dtype=np.uint8)
    got, st = ctypes.c_size_t(0), N.InflateStats()
    N.check(lib.kbbq_inflate_bgzf(dev.context().handle, N.ptr(src) if len(src) else None, len(src), N.ptr(out) if len(out) else None,
                                  len(out), ctypes.byref(got), ctypes.byref(st)))
    if stats is not None:
        stats.update({k: int(getattr(st, k)) for k, _ in N.InflateStats._fields_})
    return out[:got.value].tobytes()


def inflate_stats():
    """What the readers (kbbq_inflate_all) have sent through the device since the process began: device_blocks, host_blocks
    (the fallback count), bytes_up, bytes_down."""
    from . import _native as N
    st = N.InflateStats()
    N.check(N.load().kbbq_inflate_stats_get(st))
    return {k: int(getattr(st, k)) for k, _ in N.InflateStats._fields_}


def wants_device(*paths):
    """Would the readers inflate one of these files on the device once a context exists?  (KBBQ_GPU_INFLATE=1, a gzip file of at
    least KBBQ_GPU_INFLATE_MIN_BYTES.)  The callers that open their input while the device warms up then warm up first."""
    if os.environ.get('KBBQ_GPU_INFLATE') != '1':
        return False
    try:
        least = int(os.environ.get('KBBQ_GPU_INFLATE_MIN_BYTES') or (1 << 20))
    except ValueError:
        least = 1 << 20
    for p in paths:
        try:
            if p is not None and os.path.getsize(p) >= max(least, 2):
                with open(p, 'rb') as fh:
                    if fh.read(2) == b'\x1f\x8b':
                        return True
        except OSError:
            pass
    return False


# ---- the option ----------------------------------------------------------------------------------------------------------
_on = [False]


def enabled():
    return _on[0]


@contextlib.contextmanager
def output(bgzf):
    """While this runs with bgzf true, the sinks below are compressed.  bgzf false changes nothing (an outer call's choice stays)."""
    if not bgzf:
        yield
        return
    saved, _on[0] = _on[0], True
    try:
        yield
    finally:
        _on[0] = saved


def option(fn):
    """fn gains the keyword `bgzf` (default False): it runs inside output(bgzf)."""
    @functools.wraps(fn)
    def run(*args, bgzf=False, **kw):
        with output(bgzf):
            return fn(*args, **kw)
    return run


def open_sink(path):
    """The binary file `path` for writing: compressed when the option is on."""
    raw = open(path, 'wb')
    if not enabled():
        return raw
    try:
        return BgzfWriter(raw, close_raw=True)
    except BaseException:
        raw.close()
        raise


def stdout_sink():
    """A compressing writer over the process's binary stdout (a context manager; stdout itself stays open)."""
    sys.stdout.flush()
    return BgzfWriter(getattr(sys.stdout, 'buffer', None))


def write_text(target, text):
    """`text` (latin-1 characters) compressed to `target`: a path, or a text stream over a binary one (sys.stdout)."""
    if isinstance(target, str):
        sink = open_sink(target)
    else:
        target.flush()
        sink = BgzfWriter(getattr(target, 'buffer', None))
    with sink:
        sink.write(text.encode('latin-1'))
