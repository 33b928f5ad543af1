"""CPU model of `kbbq correct --partitions P` (kbbq/kmer.py "Partitions", include/kbbq_hip.h): the keys of tests/kmer_model.py's
exact count split by an independent restatement of the owner function, the per-partition histograms summed, and the pairs
with count >= keep united.  A test helper only.  Also F, the read set the partition tests share."""
import numpy as np

import kmer_model as M

M64 = (1 << 64) - 1
SALT = 0x9E3779B97F4A7C15

FIXTURE = dict(genome_len=20000, depth=30, err=0.01, len_lo=36, len_hi=300)      # F = M.synth(7, **FIXTURE): 3571 reads
# (windows, distinct keys, keys of count >= 2, threshold) of F on the CPU model
FIGURES = {31: (492313, 144905, 22594, 5), 21: (528023, 115814, 22607, 6)}
LARGEST = {31: {2: 72527, 3: 48514, 8: 18259, 64: 2370}}                        # keys of the largest partition at k = 31

_memo = {}


def fixture():
    """(seq plane, meta) of F, made once and read-only."""
    if 'F' not in _memo:
        seq, meta = M.synth(7, **FIXTURE)[:2]
        seq.setflags(write=False)
        meta.setflags(write=False)
        _memo['F'] = (seq, meta)
    return _memo['F']


def counted(k):
    """M.count of F at k, once."""
    if k not in _memo:
        keys, counts = M.count(*fixture(), k)
        keys.setflags(write=False)
        counts.setflags(write=False)
        _memo[k] = (keys, counts)
    return _memo[k]


def mix_int(x):
    """The 64-bit mix of one Python int, every step wrapped by hand."""
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def part_int(key, P):
    """part(key, P) of one Python int: the high half of mix(key ^ SALT), scaled to 0..P-1."""
    return ((mix_int((int(key) ^ SALT) & M64) >> 32) * int(P)) >> 32


def part(keys, P):
    """part(key, P) of an array of keys.  The 64-bit products are built from 32-bit halves in Python-int-free uint64
    arithmetic that never overflows silently: (a * b) mod 2^64 = lo(a) * b_lo + ((lo(a) * b_hi + hi(a) * b_lo) << 32)."""
    x = np.asarray(keys, dtype=np.uint64) ^ np.uint64(SALT)
    lo32 = np.uint64(0xFFFFFFFF)

    def mul(a, c):
        c_lo, c_hi = np.uint64(c & 0xFFFFFFFF), np.uint64(c >> 32)
        a_lo, a_hi = a & lo32, a >> np.uint64(32)
        with np.errstate(over='ignore'):
            cross = (a_lo * c_hi + a_hi * c_lo) & lo32
            return a_lo * c_lo + (cross << np.uint64(32))
    x = x ^ (x >> np.uint64(30))
    x = mul(x, 0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = mul(x, 0x94d049bb133111eb)
    x = x ^ (x >> np.uint64(31))
    return (((x >> np.uint64(32)) * np.uint64(int(P))) >> np.uint64(32)).astype(np.int64)


def partition(keys, counts, P, p):
    """(keys, counts) of partition p of P, sorted by key as `keys` is."""
    mine = part(keys, P) == p
    return keys[mine], counts[mine]


def rounds(keys, counts, P, keep):
    """What P rounds leave: (summed histogram, kept keys sorted, their counts, keys of the largest partition)."""
    owner = part(keys, P)
    hist = np.zeros(257, dtype=np.int64)
    kk, kc, largest = [], [], 0
    for p in range(P):
        mine = owner == p
        largest = max(largest, int(mine.sum()))
        hist += M.histogram(counts[mine])
        keep_p = mine & (counts >= keep)
        kk.append(keys[keep_p])
        kc.append(counts[keep_p])
    kk, kc = np.concatenate(kk), np.concatenate(kc)
    order = np.argsort(kk, kind='stable')
    return hist, kk[order], kc[order], largest
