"""CPU model of the k-mer set file (kbbq/kmerset.py, version 1), built on kmer_model and kmer_gate_model: the canonical k-mers of a
list of (sequence, qualities) records counted by those models' own definitions, the pairs with count >= keep sorted by unsigned
key, the histogram zeroed below keep, the two sums, and the file's bytes written out field by field.  check_pairs is the
statement of what the device check (kbbq_kmer_check_pairs_dev) enforces.  A test helper only."""
import struct

import numpy as np

import kmer_gate_model as G
import kmer_model as M

MAGIC, VERSION, HEADER_BYTES = b'KBBQKMER', 1, 2120
ORDER, RANGE, CANONICAL, COUNT = 1, 2, 3, 4          # the reasons, in the order they are tried (KBBQ_KMER_PAIR_*)
_MASK = (1 << 64) - 1


def planes(records):
    """(seq plane, qual plane, meta) of (sequence bytes, quality characters or None) records: padding 'N' / byte 0."""
    seq, meta = M.plane([s for s, _ in records])
    qual = np.zeros(seq.shape, dtype=np.uint8)
    for i, (s, q) in enumerate(records):
        if q is not None:
            assert len(q) == len(s)
            qual[i, :len(q)] = np.frombuffer(q, dtype=np.uint8)
    return seq, qual, meta


def count(records, k, Q=None):
    """(keys uint64 ascending, counts int64) of every counted window of the records; Q: the quality gate (characters at 33)."""
    if not records:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    seq, qual, meta = planes(records)
    return G.count(seq, qual, meta, k, Q + 33) if Q is not None else M.count(seq, meta, k)


def kept(records, k, keep, Q=None):
    """(keys, counts, hist, windows): the pairs with count >= keep, the histogram with zeros below keep, the counted windows."""
    keys, counts = count(records, k, Q)
    hist = M.histogram(counts)
    hist[:keep] = 0
    sel = counts >= keep
    return keys[sel], counts[sel], hist, int(counts.sum())


def file_bytes(k, keep, min_qual, reads, windows, hist, keys, counts, key_sum=None, count_sum=None):
    """The file of these fields, field by field as the format's table lists them."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.int64)
    if key_sum is None:
        key_sum = sum(int(x) for x in keys.tolist()) & _MASK
    if count_sum is None:
        count_sum = int(counts.sum()) & _MASK
    out = MAGIC + struct.pack('<IIII', VERSION, k, keep, min_qual) + struct.pack('<QQQQQ', len(keys), reads, windows, key_sum, count_sum)
    out += b''.join(struct.pack('<Q', int(h)) for h in hist)
    assert len(out) == HEADER_BYTES
    out += b''.join(struct.pack('<Q', int(x)) for x in keys.tolist())
    out += b''.join(struct.pack('<I', int(c)) for c in counts.tolist())
    assert len(out) == HEADER_BYTES + 12 * len(keys)
    return out


def set_bytes(records, k, keep, Q=None, reads=None):
    """The bytes `kbbq count` must write for these records (reads: the records read, when some of them were left out)."""
    keys, counts, hist, windows = kept(records, k, keep, Q)
    return file_bytes(k, keep, Q or 0, len(records) if reads is None else reads, windows, hist, keys, counts)


def parse(data):
    """A dict of every field of a file's bytes (keys uint64, counts uint32, hist int64)."""
    version, k, keep, min_qual = struct.unpack_from('<IIII', data, 8)
    n, reads, windows, key_sum, count_sum = struct.unpack_from('<QQQQQ', data, 24)
    hist = np.frombuffer(data, dtype='<u8', count=257, offset=64).astype(np.int64)
    keys = np.frombuffer(data, dtype='<u8', count=n, offset=HEADER_BYTES)
    counts = np.frombuffer(data, dtype='<u4', count=n, offset=HEADER_BYTES + 8 * n)
    return dict(magic=data[:8], version=version, k=k, keep=keep, min_qual=min_qual, n=n, reads=reads, windows=windows,
                key_sum=key_sum, count_sum=count_sum, hist=hist, keys=keys, counts=counts)


def check_pairs(keys, counts, k, keep, key_sum, count_sum):
    """What a loader must find: (index, reason) of the lowest pair that breaks a rule -- not above the key before it, not below
    4^k, not canonical, count below keep, tried in that order -- else 'checksum' when a sum differs, else None."""
    before = None
    for i, (key, c) in enumerate(zip((int(x) for x in np.asarray(keys).tolist()), (int(x) for x in np.asarray(counts).tolist()))):
        if before is not None and key <= before:
            return i, ORDER
        if key >= 4 ** k:
            return i, RANGE
        if key > M.revcomp(key, k):
            return i, CANONICAL
        if c < keep:
            return i, COUNT
        before = key
    if (sum(int(x) for x in np.asarray(keys).tolist()) & _MASK, sum(int(x) for x in np.asarray(counts).tolist()) & _MASK) \
            != (key_sum, count_sum):
        return 'checksum'
    return None


def retouch(data, keys=None, counts=None, fix_sums=True):
    """A file's bytes with other pairs (same n) and, with fix_sums, the header's sums made to fit them: what a tampering test needs
    to get past the header to the pair check.  hist is left alone (n does not change)."""
    f = parse(data)
    keys = f['keys'] if keys is None else np.asarray(keys, dtype=np.uint64)
    counts = f['counts'] if counts is None else np.asarray(counts, dtype=np.uint32)
    assert len(keys) == len(counts) == f['n']
    return file_bytes(f['k'], f['keep'], f['min_qual'], f['reads'], f['windows'], f['hist'], keys, counts,
                      None if fix_sums else f['key_sum'], None if fix_sums else f['count_sum'])
