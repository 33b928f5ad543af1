"""
Cells and tables for the model solve (K3) at which rounding, the tie-break or the edge of the binomial's support decides
the answer, with a reference that shares nothing with the product: plain NumPy, SciPy, `decimal` and the oracle.  Seeded and
cached per process; the host tests (test_solve_cases_host.py) and the GPU tests (test_gpu_solve_reference.py) use the same
arrays, which are read-only.

The reference of a cell is oracle.gatk_delta_q: SciPy's float64 binom.logpmf added to a longdouble prior, first maximum
wins.  Random cells never come near a decision by rounding (the best and second-best posterior of 200,000 random cells
differ by > 2e-5), so directed_cells() searches for them; each cell found is tagged by the wrong kernels it would expose.
"""
import decimal
import functools
import types

import numpy as np
import scipy.special
import scipy.stats

import oracle as O

NQ = 43
KINDS = ('double_add', 'fused', 'last_max', 'assoc')          # (a), (b), (c), (d) of terms_argmaxes()
MAX_TOTAL = 30_000_000_000                                     # the domain: 0 <= errs <= total < 3e10


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def consts():
    """(prior longdouble[43], logp[43], log1mp[43]): the oracle's prior and the two SciPy tables binom._logpmf multiplies."""
    p = O.q_to_p(np.arange(NQ)).astype(np.float64)
    with np.errstate(divide='ignore'):
        return _frozen(O.PRIOR_DIST), _frozen(scipy.special.xlogy(1.0, p)), _frozen(scipy.special.xlog1py(1.0, -p))


def comb_scipy(errs, total):
    """The candidate-independent term of logpmf(errs + 1; total + 2, p) as SciPy forms it (binom_gen._logpmf)."""
    k = np.asarray(errs, dtype=np.int64) + 1.0
    n = np.asarray(total, dtype=np.int64) + 2.0
    with np.errstate(all='ignore'):
        return scipy.special.gammaln(n + 1) - (scipy.special.gammaln(k + 1) + scipy.special.gammaln(n - k + 1))


def loglike(errs, total):
    """binom.logpmf(errs + 1; total + 2, 10^(-q'/10)) for q' = 0..42, [43, n] float64, spelled out as SciPy evaluates it inside
    the support: (comb + xlogy(k, p)) + xlog1py(n - k, -p), where x * log for x != 0 and 0 for x == 0."""
    _, logp, log1mp = consts()
    k = (np.asarray(errs, dtype=np.int64) + 1).astype(np.float64)
    nk = (np.asarray(total, dtype=np.int64) + 2).astype(np.float64) - k
    with np.errstate(all='ignore'):
        t1 = np.where(k == 0, 0.0, k * logp[:, None])
        t2 = np.where(nk == 0, 0.0, nk * log1mp[:, None])
        return (comb_scipy(errs, total) + t1) + t2, t1, t2


def terms_argmaxes(prior_q, errs, total):
    """The reference's argmax restated in NumPy, and the argmax of four WRONG kernels on the same terms:
         double_add (a) the final add of prior and log-likelihood done in float64, not in longdouble
         fused      (b) the two products kept in longdouble until each sum rounds (a fused multiply-add)
         last_max   (c) the last maximum wins instead of the first: differs exactly on an exact tie
         assoc      (d) the sum associated as comb + (t1 + t2)
    Returns (reference argmax [n], {kind: bool[n] -- that wrong kernel answers differently})."""
    prior, logp, log1mp = consts()
    prior_q = np.asarray(prior_q, dtype=np.int64)
    pr = prior[np.abs(np.arange(NQ)[:, None] - prior_q)]
    ll, t1, t2 = loglike(errs, total)
    comb = comb_scipy(errs, total)
    k = (np.asarray(errs, dtype=np.int64) + 1).astype(np.longdouble)
    nk = (np.asarray(total, dtype=np.int64) + 2).astype(np.longdouble) - k
    with np.errstate(all='ignore'):
        post = pr + ll
        ref = np.argmax(post, axis=0)
        wrong = {
            'double_add': np.argmax(pr.astype(np.float64) + ll, axis=0),
            'last_max': NQ - 1 - np.argmax(post[::-1], axis=0),
            'assoc': np.argmax(pr + (comb + (t1 + t2)), axis=0),
        }
        s1 = (comb.astype(np.longdouble) + np.where(k == 0, 0, k * logp[:, None].astype(np.longdouble))).astype(np.float64)
        s2 = (s1.astype(np.longdouble) + np.where(nk == 0, 0, nk * log1mp[:, None].astype(np.longdouble))).astype(np.float64)
        wrong['fused'] = np.argmax(pr + s2, axis=0)
    return ref, {name: wrong[name] != ref for name in KINDS}


def _cells(prior_q, errs, total):
    c = types.SimpleNamespace(prior_q=_frozen(np.asarray(prior_q, dtype=np.int64)), errs=_frozen(np.asarray(errs, dtype=np.int64)),
                              total=_frozen(np.asarray(total, dtype=np.int64)))
    c.dq = _frozen(O.gatk_delta_q(c.prior_q, c.errs, c.total))
    return c


DRAWS, SHORTLIST, KEEP, REACH = 300_000, 240, 40, 8


@functools.lru_cache(maxsize=None)
def directed_cells():
    """Cells whose two best candidates are separated by nothing, or by less than one rounding.  For every prior 0..42 and every
    pair of neighbouring candidates (c, c + 1) within REACH of it: draw errs + 1 log-uniformly, solve
        dprior + k * dlogp + nk * dlog1mp = 0
    for nk = total - errs + 1, round it to an integer, shortlist the SHORTLIST draws whose remaining difference is smallest in
    float64, evaluate those in the reference's own arithmetic and keep the KEEP with the smallest |posterior[c] - posterior[c+1]|
    there.  Fields: prior_q, errs, total, dq (= oracle.gatk_delta_q), tie (exact tie of the maximum) and one bool array per
    KINDS entry; `tagged` = any of them."""
    prior, logp, log1mp = consts()
    rng = np.random.default_rng(20250611)
    k = np.unique(np.floor(10 ** rng.uniform(0, 9.5, DRAWS)))
    pq_l, e_l, t_l, c_l = [], [], [], []
    for pq in range(NQ):
        for c in range(max(1, pq - REACH), min(NQ - 1, pq + REACH)):          # candidate 0 has log1mp = -inf: no root
            dpr = float(prior[abs(c - pq)] - prior[abs(c + 1 - pq)])
            dlp, dl1 = logp[c] - logp[c + 1], log1mp[c] - log1mp[c + 1]
            root = -(dpr + k * dlp) / dl1
            nk = np.rint(root)
            ok = (nk >= 1) & (k - 1 + nk - 1 < MAX_TOTAL)
            kk, nk, res = k[ok], nk[ok], (np.abs(nk - root) * abs(dl1))[ok]
            if kk.size > SHORTLIST:
                sel = np.argpartition(res, SHORTLIST)[:SHORTLIST]
                kk, nk = kk[sel], nk[sel]
            errs = (kk - 1).astype(np.int64)
            pq_l.append(np.full(errs.size, pq)); e_l.append(errs); t_l.append(errs + nk.astype(np.int64) - 1)
            c_l.append(np.full(errs.size, c))
    pq, errs, total, cand = (np.concatenate(x) for x in (pq_l, e_l, t_l, c_l))
    assert np.all((0 <= errs) & (errs <= total) & (total < MAX_TOTAL))
    # the shortlist in the reference's arithmetic: the gap between the pair, and whether the pair is the maximum at all
    ll, _, _ = loglike(errs, total)
    post = prior[np.abs(np.arange(NQ)[:, None] - pq)] + ll
    col = np.arange(pq.size)
    gap = np.abs(post[cand, col] - post[cand + 1, col])
    gap[post.max(axis=0) != np.maximum(post[cand, col], post[cand + 1, col])] = np.inf
    keep = []
    start = 0
    for n in (x.size for x in pq_l):
        idx = start + np.argsort(gap[start:start + n], kind='stable')[:KEEP]
        keep.append(idx[np.isfinite(gap[idx])])
        start += n
    keep = np.concatenate(keep)
    _, first = np.unique(np.stack([pq[keep], errs[keep], total[keep]]), axis=1, return_index=True)
    keep = keep[np.sort(first)]
    cells = _cells(pq[keep], errs[keep], total[keep])
    ref, kinds = terms_argmaxes(cells.prior_q, cells.errs, cells.total)
    cells.ref = _frozen(ref)
    for name in KINDS:
        setattr(cells, name, _frozen(kinds[name]))
    cells.tie = cells.last_max
    cells.tagged = _frozen(np.logical_or.reduce([kinds[name] for name in KINDS]))
    return cells


def floors(cells):
    """What the directed set holds, for the tests' floors and the log."""
    f = {'cells': int(cells.prior_q.size), 'min_per_prior': int(np.bincount(cells.prior_q, minlength=NQ).min()),
         'ties': int(cells.tie.sum())}
    f.update({name: int(getattr(cells, name).sum()) for name in KINDS})
    return f


@functools.lru_cache(maxsize=None)
def boundary_cells():
    """The edges of the binomial's support, k = errs + 1 against n = total + 2: k < 0, k == 0, k == n - 1, k == n, k > n, n < 0,
    n == 0, at a prior from each regime of the prior table (0, inside, 18 | 19 = its last finite | first -inf distance, 42)."""
    pq, errs, total = [], [], []
    for t in (-5, -3, -2, -1, 0, 1, 2, 7, 1000):
        for e in (-4, -2, -1, 0, t - 1, t, t + 1, t + 2, t + 9):
            for p in (0, 1, 10, 18, 19, 25, 42):
                pq.append(p); errs.append(e); total.append(t)
    return _cells(pq, errs, total)


def _meanq_decimal(q_total):
    """meanq per read group with 50 digits: -10 log10(sum_q q_total * p[q] / total), p[q] the reference's float64 10^(-q/10) taken
    exactly; returns (truncated and clipped to 0..42, distance of the untruncated value to the nearest integer)."""
    p = [decimal.Decimal(float(x)) for x in O.q_to_p(np.arange(NQ)).astype(np.float64)]
    meanq, dist = [], []
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        for row in q_total:
            tot = sum(int(x) for x in row)
            v = -10 * (sum(int(x) * p[q] for q, x in enumerate(row)) / tot).log10()
            meanq.append(min(max(int(v), 0), NQ - 1))                      # int(): toward zero, as the reference truncates
            dist.append(float(abs(v - v.to_integral_value())))
    return np.array(meanq, dtype=np.int64), np.array(dist)


def _finish(pos_errs, pos_total, dinuc_errs, dinuc_total, meanq):
    t = types.SimpleNamespace(R=pos_errs.shape[0], S2=pos_errs.shape[2])
    q_errs, q_total = pos_errs.sum(axis=2), pos_total.sum(axis=2)
    rg_errs, rg_total = q_errs.sum(axis=1), q_total.sum(axis=1)
    t.vectors = tuple(_frozen(x) for x in (meanq, rg_errs, rg_total, q_errs, q_total, pos_errs, pos_total, dinuc_errs, dinuc_total))
    t.dqs = tuple(_frozen(x) for x in O.get_delta_qs(*t.vectors))           # rgdq, qdq, posdq, dinucdq
    t.prior2 = _frozen((meanq + t.dqs[0])[:, None] + t.dqs[1])              # the prior of the cycle and dinucleotide cells of row (r, q)
    t.flat = _frozen(np.concatenate([x.ravel() for x in t.vectors[5:]]))    # the device's table buffer
    return t


@functools.lru_cache(maxsize=None)
def tables(R, S2, seed, scale=10.3):
    """Adversarial count tables [R, 43, S2] and [R, 43, 16]: counts log-uniform up to 10^scale (2e10), a tenth of the cells
    empty, a twentieth with errs == total, error rates from 1 to 1e-5 -- with the reference's vectors and delta tables built
    without kbbq._solve: marginals by NumPy sums, meanq in `decimal`, oracle.get_delta_qs.  Redrawn until every read group
    counts at least two qualities and its meanq lies >= 1e-6 from an integer (the kernel hands over to the host within 1e-7)."""
    rng = np.random.default_rng([seed, R, S2])

    def cells(shape):
        n = int(np.prod(shape))
        tot = (10 ** rng.uniform(0, scale, n)).astype(np.int64)
        err = np.minimum((tot * 10 ** (-rng.uniform(0, 5, n))).astype(np.int64), tot)
        u = rng.random(n)
        tot[u < 0.1] = 0; err[u < 0.1] = 0
        err[(u > 0.1) & (u < 0.15)] = tot[(u > 0.1) & (u < 0.15)]
        return err.reshape(shape), tot.reshape(shape)
    for _ in range(100):
        pe, pt = cells((R, NQ, S2))
        de, dt = cells((R, NQ, 16))
        q_total = pt.sum(axis=2)
        if np.any((q_total != 0).sum(axis=1) < 2):
            continue
        meanq, dist = _meanq_decimal(q_total)
        if np.all(dist >= 1e-6):
            return _finish(pe, pt, de, dt, meanq)
    raise AssertionError('no decidable tables in 100 draws')


def with_dinuc(t, cells):
    """`t` with its dinucleotide table overwritten by `cells`.  The dinucleotide counts enter no marginal, so meanq, the first
    three delta tables and the priors t.prior2 stay put.  Cells that have a `tagged` field (directed_cells) are placed by
    prior: row (r, q) takes the next 16 cells of the prior it solves with, tagged ones first, wrapping round; other cells
    (boundary_cells) fill the rows in rotation, the row's own prior taking the place of theirs.  `placed` = indices into
    `cells`, [R, 43, 16]."""
    placed = np.empty((t.R, NQ, 16), dtype=np.int64)
    if hasattr(cells, 'tagged'):
        order = np.argsort(~cells.tagged, kind='stable')
        by_prior = [order[cells.prior_q[order] == p] for p in range(NQ)]
        cursor = [0] * NQ
        for r in range(t.R):
            for q in range(NQ):
                p = int(t.prior2[r, q])
                placed[r, q] = by_prior[p][(cursor[p] + np.arange(16)) % by_prior[p].size]
                cursor[p] += 16
    else:
        _, uniq = np.unique(np.stack([cells.errs, cells.total]), axis=1, return_index=True)
        uniq = np.sort(uniq)
        placed[:] = uniq[np.arange(placed.size) % uniq.size].reshape(placed.shape)
    v = t.vectors
    out = _finish(v[5], v[6], cells.errs[placed], cells.total[placed], v[0])
    assert np.array_equal(out.prior2, t.prior2)
    out.placed = _frozen(placed)
    return out
