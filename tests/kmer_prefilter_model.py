"""CPU model of the k-mer prefilter (include/kbbq_hip.h, "prefilter"; kbbq/kmer.py KmerFilter): the hash restated in plain
Python integers and NumPy, independent of kbbq.kmer.filter_index, the `seen` array the device must produce, and a sequential
simulation of pass 1 for the bounds the GPU tests hold `twice` and the table to.  A test helper only."""
import numpy as np

import kmer_model as M

SALT = 0xD6E8FEB86659FD93
_M64 = (1 << 64) - 1


def mix(x):
    """The table's slot hash of one Python integer."""
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & _M64
    return x ^ (x >> 31)


def index_one(key, words):
    """(word, mask) of one key, in Python integers."""
    h = mix((int(key) ^ SALT) & _M64)
    mask = 0
    for j in range(4):
        mask |= 1 << ((h >> (6 * j)) & 63)
    return (h >> 24) & (words - 1), mask


def filter_index(keys, words):
    """(word int64, mask uint64) of every key: the same in NumPy, written out step by step."""
    x = np.asarray(keys, dtype=np.uint64) ^ np.uint64(SALT)
    with np.errstate(over='ignore'):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94d049bb133111eb)
        h = x ^ (x >> np.uint64(31))
    one = np.uint64(1)
    mask = (one << (h & np.uint64(63))) | (one << ((h >> np.uint64(6)) & np.uint64(63))) \
        | (one << ((h >> np.uint64(12)) & np.uint64(63))) | (one << ((h >> np.uint64(18)) & np.uint64(63)))
    return ((h >> np.uint64(24)) & np.uint64(words - 1)).astype(np.int64), mask


def filter_words(total, bits=4):
    words = 1
    while words * 64 < bits * total:
        words *= 2
    return words


def seen_expected(keys, words):
    """`seen` after pass 1 over any multiset of these distinct keys: the OR of their masks, word by word."""
    word, mask = filter_index(keys, words)
    seen = np.zeros(words, dtype=np.uint64)
    np.bitwise_or.at(seen, word, mask)
    return seen


def stream(seq, meta, k, order=None):
    """The canonical keys of every valid window in read order (rows in `order` when given)."""
    _, canon, valid = M.windows(seq, meta, k)
    if order is not None:
        canon, valid = canon[order], valid[order]
    return canon[valid]


def simulate(keys_in_order, words):
    """Pass 1 run sequentially: (seen, twice, admitted) as the contract states it, one window after the other."""
    word, mask = filter_index(keys_in_order, words)
    seen = [0] * words
    twice = [0] * words
    admitted = 0
    for w, m in zip(word.tolist(), mask.tolist()):
        before = seen[w]
        seen[w] = before | m
        if before & m != m:
            continue
        before = twice[w]
        twice[w] = before | m
        if before & m != m:
            admitted += 1
    return np.array(seen, dtype=np.uint64), np.array(twice, dtype=np.uint64), admitted


def in_filter(keys, array):
    """Which keys have their whole mask in `array` (seen or twice)."""
    word, mask = filter_index(keys, array.size)
    return (array[word] & mask) == mask
