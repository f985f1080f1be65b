"""numpy restatement of "ranks of pairs" (include/f2v.h: f2v_pair_ranks; tests/test_pair_ranks.py, tools/pair_ranks_time.py).  The full
score row of every query vertex comes from nearest_ref.scores, the order word W from the definition's formula, the filter sets from
the CSR as Python sets, and the summary formulas are written out here, independently of the C code.  Nothing here knows how the
kernels tile, split, count or correct."""
import numpy as np

import nearest_ref as N

EXCLUDE_SELF, EXCLUDE_NEIGHBOURS = 1, 2
BLOCK = 1024  # pairs per block of the mrr sum


def words(s):
    """W(s) of a float32 array: 0 for a NaN; otherwise with b = bits(s + 0.0f): ~b where the sign bit is set, else b | 0x80000000."""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        b = (s + np.float32(0.0)).astype(np.float32).view(np.uint32)
    w = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    w[np.isnan(s)] = 0
    return w


def excluded(rowptr, colids, u, v, flags):
    """E(u, v) as a Python set: {u} under EXCLUDE_SELF, the distinct ids of CSR row u under EXCLUDE_NEIGHBOURS, v always removed."""
    E = set()
    if flags & EXCLUDE_SELF:
        E.add(int(u))
    if flags & EXCLUDE_NEIGHBOURS:
        E.update(int(c) for c in colids[rowptr[u]:rowptr[u + 1]])
    E.discard(int(v))
    return E


def score_rows(X, us, metric):
    """{u: the float32 scores of row u against every row} for the distinct vertices of `us`."""
    uu = np.unique(np.asarray(us, dtype=np.int64))
    S = N.scores(X[uu], X, metric)
    return {int(u): S[i] for i, u in enumerate(uu)}


def pair_ranks(X, rowptr, colids, u, v, metric, flags, rows=None):
    """-> (greater uint32[m], equal uint32[m], candidates: the sum of |C|).  `rows`: score_rows of (at least) the u's, to share."""
    n = X.shape[0]
    rows = score_rows(X, u, metric) if rows is None else rows
    greater, equal, total = np.zeros(len(u), dtype=np.uint32), np.zeros(len(u), dtype=np.uint32), 0
    for i, (a, b) in enumerate(zip(u, v)):
        a, b = int(a), int(b)
        W = words(rows[a])
        C = np.ones(n, dtype=bool)
        C[np.array(sorted(excluded(rowptr, colids, a, b, flags)), dtype=np.int64)] = False
        C[b] = False
        greater[i] = int((W[C] > W[b]).sum())
        equal[i] = int((W[C] == W[b]).sum())
        total += int(C.sum())
    return greater, equal, total


def summary(greater, equal, ks=()):
    """The summary of the definition from the integers -> dict(rank2_sum, mean_rank, mrr, hits: {K: count}, tied_pairs).  rank2 = 2 + 2
    greater + equal (Python integers); mrr: the terms 2.0 / rank2 in input order, blocks of 1024 each summed from +0, the block sums
    added in ascending order, divided by m."""
    rank2 = [2 + 2 * int(g) + int(e) for g, e in zip(greater, equal)]
    m = len(rank2)
    total = 0.0
    for b0 in range(0, m, BLOCK):
        block = 0.0
        for r in rank2[b0:b0 + BLOCK]:
            block += 2.0 / float(r)
        total += block
    return dict(rank2_sum=sum(rank2), mean_rank=float(sum(rank2)) / (2.0 * m) if m else 0.0, mrr=total / float(m) if m else 0.0,
                hits={int(k): sum(1 for r in rank2 if r <= 2 * int(k)) for k in ks}, tied_pairs=sum(1 for e in equal if int(e) > 0))


def heldout_pairs(held_u, held_v, sample=None, both_ends=True):
    """The pair lists of Engine.heldout_ranks, written out: with 0 < sample < H the edges of index floor(j H / sample), j < sample; each
    edge {a, b} gives (a, b) and, with both_ends, (b, a) behind it."""
    H = len(held_u)
    pick = range(H) if sample is None or not 0 < sample < H else [j * H // sample for j in range(sample)]
    u, v = [], []
    for e in pick:
        u.append(int(held_u[e]))
        v.append(int(held_v[e]))
        if both_ends:
            u.append(int(held_v[e]))
            v.append(int(held_u[e]))
    return np.array(u, dtype=np.uint32), np.array(v, dtype=np.uint32)
