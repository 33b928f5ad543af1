"""CPU model of kbbq correct's contract (include/kbbq_hip.h, kbbq/kmer.py): exact k-mer counts with np.unique on canonical
uint64 codes, the count histogram, the first-valley threshold and the single-substitution rule, one plain loop over the
untrusted bases.  A test helper only: the product has no CPU fallback.  Also the synthetic read sets the GPU tests use."""
import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _b in enumerate(b'ACGT'):
    _CODE[_b] = _i
LETTERS = b'ACGT'


def _codes(seq, meta):
    """Base codes 0..3, 4 for a break (anything but uppercase ACGT, and every byte at or beyond the read's length)."""
    seq = np.asarray(seq, dtype=np.uint8)
    lens = np.asarray(meta, dtype=np.uint32).astype(np.int64) & 0xFFFF
    c = _CODE[seq]
    c[np.arange(seq.shape[1])[None, :] >= lens[:, None]] = 4
    return c


def revcomp(code, k):
    r = 0
    for i in range(k):
        r = (r << 2) | (3 - ((code >> (2 * i)) & 3))
    return r


def windows(seq, meta, k):
    """(forward uint64 [n, W], canonical uint64 [n, W], valid bool [n, W]) of the windows starting at 0..W-1, W = pitch - k + 1."""
    c = _codes(seq, meta)
    n, pitch = c.shape
    W = max(pitch - k + 1, 0)
    fwd = np.zeros((n, W), dtype=np.uint64)
    rc = np.zeros((n, W), dtype=np.uint64)
    for i in range(k):
        x = (c[:, i:i + W] & 3).astype(np.uint64)
        fwd = (fwd << np.uint64(2)) | x
        rc = rc | ((np.uint64(3) - x) << np.uint64(2 * i))
    brk = np.zeros((n, pitch + 1), dtype=np.int64)
    np.cumsum(c == 4, axis=1, out=brk[:, 1:])
    valid = (brk[:, k:k + W] - brk[:, :W]) == 0
    return fwd, np.minimum(fwd, rc), valid


def count(seq, meta, k):
    """(keys uint64 sorted, counts int64) of every k-mer of the rows."""
    _, canon, valid = windows(seq, meta, k)
    keys, counts = np.unique(canon[valid], return_counts=True)
    return keys, counts.astype(np.int64)


def histogram(counts):
    h = np.zeros(257, dtype=np.int64)
    np.add.at(h, np.minimum(np.asarray(counts, dtype=np.int64), 256), 1)
    h[0] = 0
    return h


def threshold(h):
    for c in range(2, 256):
        if h[c] <= h[c + 1]:
            return c
    raise ValueError('no valley: give min_count')


def correct(seq, meta, k, t=None):
    """(corrected plane, per-read changed counts, t)."""
    seq = np.asarray(seq, dtype=np.uint8)
    keys, counts = count(seq, meta, k)
    if t is None:
        t = threshold(histogram(counts))
    solid_keys = keys[counts >= t]

    def is_solid(canon):
        i = np.searchsorted(solid_keys, canon)
        return (i < solid_keys.size) & (solid_keys[np.minimum(i, max(solid_keys.size - 1, 0))] == canon) if solid_keys.size \
            else np.zeros(np.shape(canon), dtype=bool)

    fwd, canon, valid = windows(seq, meta, k)
    c = _codes(seq, meta)
    n, pitch = seq.shape
    W = fwd.shape[1]
    solid = valid & is_solid(canon)
    out = seq.copy()
    changed = np.zeros(n, dtype=np.int64)
    if W == 0:
        return out, changed, t
    cs_s = np.zeros((n, W + 1), dtype=np.int64)
    cs_v = np.zeros((n, W + 1), dtype=np.int64)
    np.cumsum(solid, axis=1, out=cs_s[:, 1:])
    np.cumsum(valid, axis=1, out=cs_v[:, 1:])
    p = np.arange(pitch)
    lo = np.maximum(p - k + 1, 0)
    hi = np.minimum(p, W - 1) + 1                    # windows [lo, hi)
    hi = np.maximum(hi, lo)
    any_s = (cs_s[:, hi] - cs_s[:, lo]) > 0
    any_v = (cs_v[:, hi] - cs_v[:, lo]) > 0
    untrusted = (c < 4) & any_v & ~any_s
    mask = (1 << (2 * k)) - 1
    solid_set = set(solid_keys.tolist())
    for r, i in zip(*np.nonzero(untrusted)):
        orig = int(c[r, i])
        cover = [j for j in range(int(lo[i]), int(hi[i])) if valid[r, j]]
        s = {}
        for b in range(4):
            if b == orig:
                continue
            tot = 0
            for j in cover:
                f = (int(fwd[r, j]) ^ ((orig ^ b) << (2 * (k - 1 - (i - j))))) & mask
                key = min(f, revcomp(f, k))
                tot += key in solid_set
            s[b] = tot
        best = max(s, key=lambda b: s[b])
        if s[best] >= 1 and sum(1 for b in s if s[b] == s[best]) == 1:
            out[r, i] = LETTERS[best]
            changed[r] += 1
    return out, changed, t


def plane(reads, pitch=None):
    """Rows of byte strings -> (seq plane padded with 'N', meta words)."""
    longest = max([len(x) for x in reads] + [1])
    pitch = pitch or max(16, (longest + 15) // 16 * 16)
    seq = np.full((len(reads), pitch), ord('N'), dtype=np.uint8)
    for i, x in enumerate(reads):
        seq[i, :len(x)] = np.frombuffer(x, dtype=np.uint8)
    return seq, np.array([len(x) for x in reads], dtype=np.uint32)


def synth(seed, genome_len=30000, depth=30, err=0.01, len_lo=36, len_hi=300, n_rate=0.001):
    """Reads from both strands of a random genome: (seq plane with errors and Ns, meta, error-free plane, error mask)."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len).astype(np.uint8)
    lens = rng.integers(len_lo, len_hi + 1, size=max(1, int(genome_len * depth / ((len_lo + len_hi) / 2))))
    pitch = max(16, (int(lens.max()) + 15) // 16 * 16)
    n = lens.size
    truth = np.full((n, pitch), ord('N'), dtype=np.uint8)
    for r, L in enumerate(lens.tolist()):
        s = int(rng.integers(0, genome_len - L + 1))
        x = genome[s:s + L]
        if rng.random() < 0.5:
            x = (3 - x)[::-1]
        truth[r, :L] = np.frombuffer(LETTERS, dtype=np.uint8)[x]
    inside = np.arange(pitch)[None, :] < lens[:, None]
    errs = inside & (rng.random((n, pitch)) < err)
    seq = truth.copy()
    shift = rng.integers(1, 4, size=(n, pitch)).astype(np.uint8)
    sub = np.frombuffer(LETTERS, dtype=np.uint8)[(_CODE[truth] + shift) % 4]
    seq[errs] = sub[errs]
    ns = inside & ~errs & (rng.random((n, pitch)) < n_rate)
    seq[ns] = ord('N')
    return seq, lens.astype(np.uint32), truth, errs
