"""CPU model of `kbbq correct --passes P` (include/kbbq_hip.h, "Passes"), written from the contract on top of kmer_model's windows
and codes: one pass of the rule against a FIXED sorted set of solid canonical keys -- the substitution rule as
kmer_unresolved_model.classify(solid_keys=...) judges it, here with the winning letter, and the N rule of kmer_fixn_model
restated against the fixed set -- and its repetition row by row.  The set comes from the reads as read and is never recounted.
A test helper only: the product has no CPU fallback.

r_0 is the row as read, r_p = C(r_(p-1)); a pass that changes nothing in a row ends that row.  The flag plane of r_P: 1 where
r_P differs from r_0, 2 where it does not and the last evaluation of the row (pass P, or the pass that found the fixed point)
left the base unresolved, 0 elsewhere."""
import numpy as np

import kmer_model as M
import kmer_fixn_model as F
import kmer_unresolved_model as U

NCH = ord('N')
_LET = np.frombuffer(M.LETTERS, dtype=np.uint8)


def solid_set(seq, meta, k, t=None):
    """(sorted uint64 solid canonical keys, t) of the rows as read."""
    keys, counts = M.count(seq, meta, k)
    if t is None:
        t = M.threshold(M.histogram(counts))
    return keys[counts >= t].astype(np.uint64), int(t)


def _is_solid(solid_keys, canon):
    if not solid_keys.size:
        return np.zeros(np.shape(canon), dtype=bool)
    i = np.minimum(np.searchsorted(solid_keys, canon), solid_keys.size - 1)
    return solid_keys[i] == canon


def one_pass(seq, meta, k, solid_keys, fix_n=False, sep=None):
    """(new plane, class plane) of one pass over every row: class 0 trusted / break / padding / N, 1 changed (a substitution, or
    with fix_n a fixed N), 2 unresolved.  Every base is judged against `seq`."""
    seq = np.asarray(seq, dtype=np.uint8)
    solid_keys = np.asarray(solid_keys, dtype=np.uint64)
    n, pitch = seq.shape
    out = seq.copy()
    cls = np.zeros((n, pitch), dtype=np.uint8)
    fwd, canon, valid = M.windows(seq, meta, k)
    W = fwd.shape[1]
    if W == 0 or n == 0:
        return out, cls
    c = M._codes(seq, meta)
    solid = valid & _is_solid(solid_keys, canon)
    cs_s = np.zeros((n, W + 1), dtype=np.int64)
    cs_v = np.zeros((n, W + 1), dtype=np.int64)
    np.cumsum(solid, axis=1, out=cs_s[:, 1:])
    np.cumsum(valid, axis=1, out=cs_v[:, 1:])
    p = np.arange(pitch)
    lo = np.maximum(p - k + 1, 0)
    hi = np.maximum(np.minimum(p, W - 1) + 1, lo)
    untrusted = (c < 4) & ((cs_v[:, hi] - cs_v[:, lo]) > 0) & ((cs_s[:, hi] - cs_s[:, lo]) == 0)
    rr, ii = np.nonzero(untrusted)
    if rr.size:
        rc = U._revcomp(fwd, k)
        score = np.zeros((rr.size, 4), dtype=np.int64)   # [:, x]: solid covering windows with the base's code XOR x written
        for d in range(k):                               # the base is the d-th base of the window starting at i - d
            j = ii - d
            ok = (j >= 0) & (j < W)
            jj = np.clip(j, 0, W - 1)
            ok &= valid[rr, jj]
            f, r = fwd[rr, jj], rc[rr, jj]
            for x in (1, 2, 3):
                ff = f ^ (np.uint64(x) << np.uint64(2 * (k - 1 - d)))
                rx = r ^ (np.uint64(x) << np.uint64(2 * d))
                score[:, x] += ok & _is_solid(solid_keys, np.minimum(ff, rx))
        top = score[:, 1:].max(axis=1)
        winner = (top >= 1) & ((score[:, 1:] == top[:, None]).sum(axis=1) == 1)
        x = score[:, 1:].argmax(axis=1) + 1
        cls[rr, ii] = np.where(winner, 1, 2)
        out[rr[winner], ii[winner]] = _LET[c[rr[winner], ii[winner]] ^ x[winner]]
    if fix_n:
        solid_py = set(solid_keys.tolist())
        lens = (np.asarray(meta, dtype=np.uint32).astype(np.int64) & 0xFFFF).tolist()
        rows, cols = np.nonzero((seq == NCH) & (p[None, :] < np.asarray(lens)[:, None]))
        for r, i in zip(rows.tolist(), cols.tolist()):
            if sep is not None and sep[r] is not None and int(sep[r]) == i:
                continue
            L = lens[r]
            cand = [s for s in range(max(0, i - k + 1), min(i, L - k) + 1) if int((c[r, s:s + k] == 4).sum()) == 1]
            if not cand:
                continue
            score = []
            for x in range(4):
                tot = 0
                for s in cand:
                    f = int(fwd[r, s]) | (x << (2 * (k - 1 - (i - s))))      # a break's code is 0 in the forward word
                    tot += min(f, F.revcomp(f, k)) in solid_py
                score.append(tot)
            best = max(score)
            if best >= 1 and score.count(best) == 1:
                out[r, i] = M.LETTERS[score.index(best)]
                cls[r, i] = 1
    return out, cls


def trace(seq, meta, k, t, P, fix_n=False, sep=None, solid_keys=None):
    """[(plane, changed, flags, ran)] after 1, 2, .. P passes: the plane r_p, the per-row count of bases where it differs from the
    rows as read, the flag plane with its 2s, and the passes each row ran so far (a row stops after the first pass that changes
    nothing in it).  solid_keys: the fixed set, else that of these rows at t (t None: the first valley)."""
    seq = np.asarray(seq, dtype=np.uint8)
    meta = np.asarray(meta, dtype=np.uint32)
    if solid_keys is None:
        solid_keys, t = solid_set(seq, meta, k, t)
    n = seq.shape[0]
    cur = seq.copy()
    last_cls = np.zeros(seq.shape, dtype=np.uint8)
    ran = np.zeros(n, dtype=np.int64)
    active = np.ones(n, dtype=bool)
    steps = []
    for _ in range(int(P)):
        idx = np.nonzero(active)[0]
        if idx.size:
            sub_sep = None if sep is None else [sep[r] for r in idx.tolist()]
            new, cls = one_pass(cur[idx], meta[idx], k, solid_keys, fix_n=fix_n, sep=sub_sep)
            moved = (new != cur[idx]).any(axis=1)
            cur[idx] = new
            last_cls[idx] = cls
            ran[idx] += 1
            active[idx] = moved
        differs = cur != seq
        flags = np.where(differs, 1, np.where(last_cls == 2, 2, 0)).astype(np.uint8)
        steps.append((cur.copy(), differs.sum(axis=1).astype(np.int64), flags, ran.copy()))
    return steps


def passes(seq, meta, k, t, P, fix_n=False, sep=None, solid_keys=None):
    """(plane r_P, changed, flag plane with 2s, passes each row ran)."""
    return trace(seq, meta, k, t, P, fix_n=fix_n, sep=sep, solid_keys=solid_keys)[-1]


# ---- hand-built rows: which pass corrects which base is known by construction ---------------------------------------------------
HAND_K, HAND_T, HAND_LEN = 11, 3, 40


def _sub(read, *at):
    x = bytearray(read)
    for i in at:
        x[i] = M.LETTERS[(M.LETTERS.index(x[i]) + 1) % 4]
    return bytes(x)


def hand_rows(pitch=48, cut=None, seed=5):
    """(seq plane, meta, cases) over a random genome of 120 bases at k = HAND_K, min_count = HAND_T: four copies of every
    40-base tile of the genome at a step of 4 (each of its k-mers is counted 4 times or more), then one read each of
        'two_pass'    g[30:70] with bases 2 and 8 substituted: windows 3..8 hold base 8 alone, windows 0..2 both -- pass 1 corrects
                      base 8, pass 2 base 2
        'three_pass'  bases 2, 5 and 9: pass 1 corrects 9 (windows 6..9), pass 2 base 5 (windows 3..5), pass 3 base 2
        'one_pass'    base 20 alone, mid-read: finished after pass 1
        'two_pass_end' / 'three_pass_end'   the same distances from the read's last base
        'truth'       g[30:70] as it is
    cases = {name: (row, (bases in the order they are corrected))}.  cut: every read is cut to its first `cut` bases."""
    rng = np.random.default_rng(seed)
    g = bytes(_LET[rng.integers(0, 4, 120)])
    L = HAND_LEN
    reads = [g[s:s + L] for s in range(0, 120 - L + 1, 4) for _ in range(4)]
    r = g[30:30 + L]
    cases = {}
    for name, at in (('truth', ()), ('two_pass', (8, 2)), ('three_pass', (9, 5, 2)), ('one_pass', (20,)),
                     ('two_pass_end', (L - 9, L - 3)), ('three_pass_end', (L - 10, L - 6, L - 3))):
        cases[name] = (len(reads), at)
        reads.append(_sub(r, *at))
    if cut is not None:
        reads = [x[:cut] for x in reads]
    seq, meta = M.plane(reads, pitch=pitch)
    return seq, meta, cases
