"""
BAM input on the device (include/kbbq_hip.h "BAM input"; csrc/bam_host.cpp kbbq_bam_scan, csrc/kbbq_bam_in.h kbd_decode).

For the commands that write no record -- `bqsr --kmers`, `count -b` -- the SAM text the host reader renders from a BAM file serves
nothing.  Here the inflated image is scanned once (header lines, @RG IDs, the chain of records), uploaded slab by slab through two
page-locked buffers, and a kernel turns the records into the resident SEQ / QUAL / OQ planes and 16 words per record.  The host
reader (kbbq.aln.AlignmentFile) decides every doubtful file: a record the kernel does not vouch for (its status word), a scan
error, a header line that is no header line, anything that is not a BGZF-compressed BAM file, a launcher's rank -- each gives
(None, reason) from open_device and the caller opens the file as it always did.  The device route never produces an answer for a
file on which it could disagree with the reader, and never words an error of its own.

Scan / slabs / decode_host need no GPU: the host twin (kbbq_bam_decode) runs the same per-record code as the kernel.
A file that falls back after its image was inflated here is inflated again by the reader: the price of asking, paid only with
the variable set.
"""
import ctypes
import os

import numpy as np

from . import _native as N

PLANES = ('seq', 'qual', 'oq')                # plane numbers 0, 1, 2 of SamBatch.plane


def stage_bytes():
    """One staging slab: KBBQ_STAGE_MB (default 96) megabytes."""
    env = os.environ.get('KBBQ_STAGE_MB', '')
    return (int(env) if env.isdigit() and int(env) > 0 else 96) << 20


def wanted(device=None):
    """device=True, or device=None with KBBQ_GPU_BAM=1."""
    return bool(device) if device is not None else os.environ.get('KBBQ_GPU_BAM') == '1'


def is_bgzf(path):
    """Does the file begin with a BGZF member (a gzip member with the BC subfield)?"""
    try:
        with open(path, 'rb') as fh:
            head = fh.read(12)
            if len(head) < 12 or head[:4] != b'\x1f\x8b\x08\x04':
                return False
            extra = fh.read(int.from_bytes(head[10:12], 'little'))
    except OSError:
        return False
    at = 0
    while at + 4 <= len(extra):
        slen = int.from_bytes(extra[at + 2:at + 4], 'little')
        if extra[at:at + 2] == b'BC' and slen == 2:
            return True
        at += 4 + slen
    return False


class Image:
    """A file's bytes, inflated by the library when it is gzip / BGZF (kbbq_text_open), as a NumPy view; close() frees them."""

    def __init__(self, path):
        from . import aln
        self._h = ctypes.c_void_p()
        data, n = ctypes.c_void_p(), ctypes.c_size_t(0)
        aln._context_for(path)
        N.check(N.load().kbbq_text_open(str(path).encode(), ctypes.byref(self._h), ctypes.byref(data), ctypes.byref(n)))
        self.bytes = (np.ctypeslib.as_array((ctypes.c_uint8 * n.value).from_address(data.value)) if n.value
                      else np.zeros(0, np.uint8))

    def close(self):
        if self._h:
            self.bytes = None
            N.load().kbbq_text_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scan:
    """kbbq_bam_scan of an inflated image (a uint8 array): n, n_ref, maxlen, header (the lines kbbq_bam_to_sam writes, as the
    reader lists them), header_ok (False when the text holds a non-blank line that is no '@' line: the reader takes it for an
    alignment), rg_ids, rg_off / rg_bytes (the table the decode reads), rec_off / cig_off (uint64), ref_names (the binary list),
    stream_bytes (records_off .. the image's end)."""

    def __init__(self, image):
        lib = N.load()
        image = np.ascontiguousarray(image, dtype=np.uint8)
        info = N.BamScanInfo()
        N.check(lib.kbbq_bam_scan(N.ptr(image), image.nbytes, ctypes.byref(info), None, None, None, None, None))
        self.n, self.n_ref, self.maxlen, self.cig_total = int(info.n), int(info.n_ref), int(info.max_l_seq), int(info.cig_total)
        header = np.zeros(max(int(info.header_bytes), 1), np.uint8)
        self.rg_off = np.zeros(int(info.n_rg) + 1, np.uint32)
        self.rg_bytes = np.zeros(max(int(info.rg_bytes), 1), np.uint8)
        self.rec_off = np.zeros(max(self.n, 1), np.uint64)
        self.cig_off = np.zeros(self.n + 1, np.uint64)
        N.check(lib.kbbq_bam_scan(N.ptr(image), image.nbytes, ctypes.byref(info), N.ptr(header), N.ptr(self.rg_off), N.ptr(self.rg_bytes),
                                  N.ptr(self.rec_off), N.ptr(self.cig_off)))
        self.rec_off = self.rec_off[:self.n]
        self.image_bytes = int(image.nbytes)
        self.records_off, self.max_record = int(info.records_off), int(info.max_record)
        self.stream_bytes = self.image_bytes - self.records_off
        # the header lines as the reader lists them: line ends and a '\r' before them removed, blank lines dropped
        self.header, self.header_ok = [], True
        for line in header[:int(info.header_bytes)].tobytes().split(b'\n'):
            if line.endswith(b'\r'):
                line = line[:-1]
            if not line.strip(b' \t'):
                continue
            if not line.startswith(b'@'):
                self.header_ok = False
            self.header.append(line.decode('latin-1'))
        rg = self.rg_bytes.tobytes()
        self.rg_ids = [rg[int(a):int(b)].decode('latin-1') for a, b in zip(self.rg_off[:-1], self.rg_off[1:])]
        at, names, raw = int(info.refs_off), [], image
        for _ in range(self.n_ref):
            l_name = int.from_bytes(raw[at:at + 4].tobytes(), 'little', signed=True)
            names.append(raw[at + 4:at + 4 + l_name - 1].tobytes().decode('latin-1'))
            at += 8 + l_name
        self.ref_names = names


def slabs(scan, slab_bytes=None):
    """[(first record, one past the last, first byte, one past the last byte)]: the stream cut at record boundaries into pieces of
    at most slab_bytes; a record larger than that is a slab of its own size."""
    slab_bytes = int(slab_bytes) if slab_bytes else stage_bytes()
    n = scan.n
    if n == 0:
        return []
    start = scan.rec_off.astype(np.int64) - 4                    # every record's block_size word
    end = np.append(start[1:], np.int64(scan.image_bytes))
    out, a = [], 0
    while a < n:
        b = int(np.searchsorted(end, start[a] + slab_bytes, side='right'))
        b = min(max(b, a + 1), n)
        out.append((a, b, int(start[a]), int(end[b - 1])))
        a = b
    return out


def _slab_tables(scan, a, b, lo):
    """(rec_off, cig_off) of a slab's records, relative to the slab, as uint32."""
    rec = (scan.rec_off[a:b].astype(np.int64) - lo).astype(np.uint32)
    cig = (scan.cig_off[a:b + 1] - scan.cig_off[a]).astype(np.uint32)
    return rec, cig


SQ_MISMATCH = 'the @SQ lines do not name the binary reference list in order'


def sq_lines_match(scan):
    """None when a record's refID means the same to the text route as to the binary list: the @SQ lines of the scan's header
    (made from the list when the text has none) name the list's references in order, each once, each with a decimal LN, none
    called '*' or '=' -- else SQ_MISMATCH.  csrc/sam_host.cpp bam_refs reads the lines the same way."""
    names = []
    for line in scan.header:
        if not line.startswith('@SQ'):
            continue
        name = length = None
        for field in line.split('\t')[1:]:
            if field.startswith('SN:'):
                name = field[3:]
            elif field.startswith('LN:'):
                length = field[3:]
        if name is None or length is None or not length.isascii() or not length.isdigit() or int(length) > 0x7FFFFFFF:
            return SQ_MISMATCH
        names.append(name)
    if names != list(scan.ref_names) or len(set(names)) != len(names) or '*' in names or '=' in names:
        return SQ_MISMATCH
    return None


def decode_host(image, scan, pitch, slab_bytes=None, planes=PLANES, cigar=True):
    """The host twin over the whole image, slab by slab like the device route: dict(seq, qual, oq: uint8 [n, pitch] or None;
    words: int32 [n, 16]; cigar: uint32 or None; status: the OR of every record's)."""
    lib = N.load()
    n = scan.n
    out = {p: (np.full((max(n, 1), pitch), 0xA5, np.uint8) if p in planes else None) for p in PLANES}   # nothing is pre-zeroed
    words = np.full((max(n, 1), 16), -1515870811, np.int32)
    ops = np.full(max(scan.cig_total, 1), 0xA5A5A5A5, np.uint32) if cigar else None
    status = 0
    for a, b, lo, hi in slabs(scan, slab_bytes):
        piece = np.ascontiguousarray(image[lo:hi])
        rec, cig = _slab_tables(scan, a, b, lo)
        any_status = ctypes.c_uint32(0)
        c0 = int(scan.cig_off[a])
        N.check(lib.kbbq_bam_decode(N.ptr(piece), piece.nbytes, N.ptr(rec), b - a, pitch, N.ptr(scan.rg_off), N.ptr(scan.rg_bytes),
                                    len(scan.rg_ids), scan.n_ref, N.ptr(cig), int(cig[-1]),
                                    *[N.ptr(out[p][a:]) if out[p] is not None else None for p in PLANES], N.ptr(words[a:]),
                                    N.ptr(ops[c0:]) if cigar else None, ctypes.byref(any_status)))
        status |= any_status.value
    out.update(words=words[:n], cigar=None if ops is None else ops[:scan.cig_total], status=status)
    for p in PLANES:
        if out[p] is not None:
            out[p] = out[p][:n]
    return out


class DeviceBatch:
    """SamBatch's attributes from the decoded words (ONE download), the planes resident on the device.  What only the text has
    -- names, lines -- comes from the host reader, opened on first use: only error messages ask for it."""

    def __init__(self, path, scan, words, planes, pitch, d_cigar):
        self._path, self._scan, self._planes, self.pitch, self._d_cigar = path, scan, planes, int(pitch), d_cigar
        self.n, self.maxlen = scan.n, scan.maxlen
        col = {name: np.ascontiguousarray(words[:, k]) for k, name in enumerate(N.BAM_WORDS)}
        self.flag, self.qlen, self.ref_span, self.rg = col['flag'], col['qlen'], col['ref_span'], col['rg']
        self.pos, self.pnext, self.tlen = (col[k].astype(np.int64) for k in ('pos', 'pnext', 'tlen'))
        self.clip, self._trim = col['clip'].view(np.uint32), col['trim'].view(np.uint32)
        self.cig_n = col['cig_n'].view(np.uint32)
        self.cig_off = scan.cig_off[:self.n].astype(np.uint32)
        self.qual_len, self.oq_len = col['qual_len'], col['oq_len']
        self.ref_id = col['ref_id']
        self.rg_ids = list(scan.rg_ids)
        self._contigs = self._cigar = self._host = None
        self.stream = None                    # a Stream: the record stream kept resident for the recode (open_device keep_stream=True)

    def _contig(self):
        """The reader's numbering: names in order of first appearance, '*' for a negative refID."""
        if self._contigs is None:
            ref = np.where(self.ref_id < 0, -1, self.ref_id)
            ids, first = np.unique(ref, return_index=True)
            names, number, of = [], {}, {}
            for i in ids[np.argsort(first, kind='stable')]:
                name = '*' if i < 0 else self._scan.ref_names[int(i)]
                if name not in number:
                    number[name] = len(names)
                    names.append(name)
                of[int(i)] = number[name]
            table = np.zeros(self._scan.n_ref + 1, np.int32)
            for i, c in of.items():
                table[i + 1] = c
            self._contigs = (table[ref + 1] if self.n else np.zeros(0, np.int32), names)
        return self._contigs

    @property
    def contig(self):
        return self._contig()[0]

    @property
    def contig_names(self):
        return self._contig()[1]

    @property
    def cigar(self):
        if self._cigar is None:
            self._cigar = (self._d_cigar.cpu().numpy().view(np.uint32)[:self._scan.cig_total] if self._scan.cig_total
                           else np.zeros(0, np.uint32))
        return self._cigar

    def adaptor_trim(self):
        return self._trim

    def device_plane(self, which, pitch):
        """The resident plane `which` (0 SEQ, 1 QUAL, 2 OQ) as a uint8 device tensor [max(n, 1), pitch]; a plane that was not
        decoded, or another pitch than the decode's, is the host copy uploaded."""
        t = self._planes.get(PLANES[which])
        if t is not None and int(pitch) == self.pitch:
            return t
        from . import _device as dev
        return dev._torch().from_numpy(np.ascontiguousarray(self.plane(which, pitch))).cuda()

    def plane(self, which, pitch, first=0, n=None):
        """SamBatch.plane: a host copy."""
        n = self.n - first if n is None else n
        t = self._planes.get(PLANES[which])
        longest = int(self.oq_len.max(initial=0)) if which == 2 else self.maxlen
        if t is None or (pitch > self.pitch and longest > self.pitch):       # not resident, or cut at the decode's pitch
            return self.reader().batch().plane(which, pitch, first, n)
        rows = t[first:first + max(n, 1)].cpu().numpy()
        out = np.zeros((max(n, 1), pitch), np.uint8)
        if n:
            w = min(pitch, self.pitch)
            out[:n, :w] = rows[:n, :w]
        return out

    def release_stream(self):
        """The resident record stream and its offsets are freed (the writer's close())."""
        self.stream = None

    def reader(self):
        if self._host is None:
            from . import aln
            self._host = aln.AlignmentFile(self._path)
        return self._host

    def _text(self, what, i):
        return self.reader().batch()._text(what, i)

    def names(self):
        return self.reader().batch().names()

    def line(self, i):
        return self.reader().batch().line(i)


class Stream:
    """The record stream of an image (records_off .. its end) in device memory, with the 64-bit offsets of the records' bodies in
    it: what kbbq_bam_recode_dev reads."""

    def __init__(self, d_bytes, d_rec_off, n_ref, maxlen, rec_off, nbytes):
        self.d_bytes, self.d_rec_off, self.n_ref, self.maxlen = d_bytes, d_rec_off, int(n_ref), int(maxlen)
        self.rec_off, self.nbytes = rec_off, int(nbytes)         # (host copy of the offsets: the skeleton's upper bound)

    def skel_cap(self, first, m, set_oq):
        """An upper bound of the skeleton of records [first, first + m): their bytes, and an OQ tag each with set_oq."""
        if m <= 0:
            return 0
        end = int(self.rec_off[first + m]) - 4 if first + m < len(self.rec_off) else self.nbytes
        return end - (int(self.rec_off[first]) - 4) + (m * (self.maxlen + 4) if set_oq else 0)


def recode_device(stream, first, m, set_oq, keep, d_stage=None, desc_bytes=0, cap=0):
    """kbbq_bam_recode_dev on records [first, first + m) of a Stream.  d_stage: a uint8 device tensor that takes the descriptors
    at its front and, from desc_bytes on, up to cap bytes of skeleton; None: no skeleton is written (the vouching pass).  keep:
    a uint8 device tensor of m bytes, or None.  (skeleton bytes, stream bytes, the OR of the status words)."""
    from . import _device as dev
    T = dev._torch()
    lib = N.load()
    d_desc = d_stage if d_stage is not None else T.empty(max(m, 1) * 4 * N.BAM_DESC_WORDS, dtype=T.uint8, device='cuda')
    d_status = T.empty(max(m, 1), dtype=T.int32, device='cuda')
    sb, tb, st = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0)
    N.check(lib.kbbq_bam_recode_dev(dev.context().handle, N.ptr(stream.d_bytes), stream.nbytes, N.ptr(stream.d_rec_off), first, m,
                                    int(bool(set_oq)), N.ptr(keep), stream.n_ref, N.ptr(d_desc),
                                    None if d_stage is None else N.ptr(d_stage.data_ptr() + desc_bytes), cap if d_stage is not None else 0,
                                    N.ptr(d_status), ctypes.byref(sb), ctypes.byref(tb), ctypes.byref(st)))
    return sb.value, tb.value, st.value


def decode_device(raw, scan, pitch, slab_bytes=None, planes=PLANES, poison=None, keep_stream=False):
    """The image's records through kbd_decode, slab by slab through two page-locked buffers: (device planes by name, device words
    int32 [n, 16], device CIGAR words, the OR of every record's status, bytes uploaded, slabs).  Stops behind the first slab with
    a status.  poison: a byte to fill every output with first (tests: the decode writes all of it).
    keep_stream: the slabs go up into ONE buffer that holds the whole record stream and stays (a Stream, returned behind the
    others); every slab is then also put to the recode's size step, whose status bits join the decode's."""
    from . import _device as dev
    T = dev._torch()
    ctx = dev.context()
    lib = N.load()
    n, rows = scan.n, max(scan.n, 1)
    d_planes = {p: T.empty((rows, pitch), dtype=T.uint8, device='cuda') for p in PLANES if p in planes}
    d_words = T.empty((rows, 16), dtype=T.int32, device='cuda')
    d_cigar = T.empty(max(scan.cig_total, 1), dtype=T.int32, device='cuda')
    up = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    if poison is not None:
        for t in list(d_planes.values()) + [d_words, d_cigar]:
            t.copy_(up(np.full(t.nbytes, poison, np.uint8)).view(t.dtype).view(t.shape))
    elif n == 0:
        for t in d_planes.values():
            t.zero_()
    d_rg_off, d_rg = up(scan.rg_off.view(np.int32)), up(scan.rg_bytes)
    cuts = slabs(scan, slab_bytes)
    room = max((hi - lo for _, _, lo, hi in cuts), default=1)
    pinned = [dev.pinned('bamin', i, room) for i in range(min(len(cuts), 2))]
    h2d = scan.rg_off.nbytes + scan.rg_bytes.nbytes
    stream = None
    if keep_stream:
        base = scan.records_off
        rel = (scan.rec_off.astype(np.int64) - base).astype(np.uint64) if n else np.zeros(1, np.uint64)
        stream = Stream(T.empty(max(scan.stream_bytes, 16), dtype=T.uint8, device='cuda'), up(rel.view(np.int64)), scan.n_ref, scan.maxlen,
                        rel[:n], scan.stream_bytes)
        h2d += rel.nbytes
    else:
        d_slab = T.empty(room, dtype=T.uint8, device='cuda')

    def fill(k):                                                      # the image's bytes into page-locked memory
        _, _, lo, hi = cuts[k]
        pinned[k % 2][:hi - lo].numpy()[:] = raw[lo:hi]
    if cuts:
        fill(0)
    status = done = 0
    for k, (a, b, lo, hi) in enumerate(cuts):
        if stream is not None:
            d_slab = stream.d_bytes[lo - base:]
        d_slab[:hi - lo].copy_(pinned[k % 2][:hi - lo], non_blocking=True)
        if k + 1 < len(cuts):
            fill(k + 1)                                               # ... the next slab's while this one goes up
        rec, cig = _slab_tables(scan, a, b, lo)
        d_rec, d_cig = up(rec.view(np.int32)), up(cig.view(np.int32))
        any_status = ctypes.c_uint32(0)
        c0 = int(scan.cig_off[a])
        N.check(lib.kbbq_bam_decode_dev(ctx.handle, N.ptr(d_slab), hi - lo, N.ptr(d_rec), b - a, pitch, N.ptr(d_rg_off), N.ptr(d_rg),
                                        len(scan.rg_ids), scan.n_ref, N.ptr(d_cig), int(cig[-1]),
                                        *[N.ptr(d_planes[p][a:]) if p in d_planes else None for p in PLANES],
                                        N.ptr(d_words[a:]), N.ptr(d_cigar[c0:]), ctypes.byref(any_status)))
        h2d += (hi - lo) + rec.nbytes + cig.nbytes
        done += 1
        status |= any_status.value
        if stream is not None and not status:
            status |= recode_device(stream, a, b - a, 0, None)[2]
        if status and poison is None:
            break
    d_slab = None
    dev.release_pinned('bamin')
    if keep_stream:
        return d_planes, d_words, d_cigar, status, h2d, done, stream
    return d_planes, d_words, d_cigar, status, h2d, done


def open_device(path, slab_bytes=None, planes=PLANES, keep_stream=False):
    """(DeviceBatch, header lines, stats) when the device route holds, else (None, None, stats) with stats['fallback'] the reason.
    keep_stream (the commands that write --bam-out): the record stream and its 64-bit offsets stay resident beside the planes
    (DeviceBatch.stream, counted against KBBQ_DEVICE_BUDGET; freed by release_stream) and the recode has to vouch for every
    record too; a header whose @SQ lines do not name the binary reference list in order is then a fallback of its own."""
    stats = dict(route='host', records=0, stream_bytes=0, h2d_bytes=0, slabs=0, fallback=None)

    def no(reason):
        stats['fallback'] = reason
        return None, None, stats
    from . import kmerset
    if kmerset._launched():
        return no('a rank of a launcher')
    if not is_bgzf(path):
        return no('not a BGZF file')
    image = Image(path)
    try:
        raw = image.bytes
        if raw.nbytes < 4 or raw[:4].tobytes() != b'BAM\1':
            return no('not a BAM stream')
        try:
            scan = Scan(raw)
        except ValueError as exc:
            return no('scan: %s' % exc)
        if not scan.header_ok:
            return no('a header line that is no header line')
        if scan.maxlen > 65535:
            return no('a record of more than 65535 bases')
        n = scan.n
        pitch = max(16, (max(scan.maxlen, 1) + 15) // 16 * 16)
        stream = None
        if keep_stream:
            if sq_lines_match(scan) is not None:
                return no(SQ_MISMATCH)
            from . import _device as dev
            need = scan.stream_bytes + 8 * n + len(planes) * max(n, 1) * pitch
            if need > dev.device_budget():
                return no('the record stream does not fit the device budget (%d bytes, KBBQ_DEVICE_BUDGET)' % need)
            d_planes, d_words, d_cigar, status, h2d, nslabs, stream = decode_device(raw, scan, pitch, slab_bytes, planes, keep_stream=True)
        else:
            d_planes, d_words, d_cigar, status, h2d, nslabs = decode_device(raw, scan, pitch, slab_bytes, planes)
        stats['slabs'] = nslabs
    finally:
        image.close()                                                 # the image is freed after the last slab
    stats.update(records=n, stream_bytes=scan.stream_bytes, h2d_bytes=h2d)
    if status:
        return no('a record the %s not vouch for (status 0x%x)' % ('decode and the recode do' if keep_stream else 'decode does', status))
    words = d_words.cpu().numpy()[:n]                                  # the one download
    del d_words
    stats['route'] = 'device'
    batch = DeviceBatch(path, scan, words, d_planes, pitch, d_cigar)
    batch.stream = stream
    return batch, scan.header, stats
