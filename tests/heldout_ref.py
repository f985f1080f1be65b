"""TEST INFRASTRUCTURE: the plain Python / numpy restatement of the three held-out link-prediction definitions of include/f2v.h,
written from the header's text: the edge split (keys, anchors, held pairs, the training CSR, the negatives), the pair scores (the
fp32 fma chains of nearest_ref) and the ranking (groups of equal score, exact integer tallies, the blocked sum of the average
precision).  Keys and tallies are Python integers.  Nothing here knows how the kernels place rows, sort or scan."""
import math
import struct

import numpy as np

from kmeans_ref import mix64
from linkpairs_ref import candidates, neighbours, u64
from nearest_ref import fma32, rnorm

U64 = np.uint64
MASK = (1 << 64) - 1
SPLIT_COUNTERS = ("edges", "candidates_held", "protected", "held", "train_nnz", "negatives", "drawn", "capped")


def seeds(seed):
    """-> (SE, SN) as Python integers"""
    s1 = int(mix64(u64(seed)))
    return int(mix64(u64(s1 ^ 0x65646765))), int(mix64(u64(s1 ^ 0x6e656773)))


def threshold(frac):
    assert 0 <= frac < 1
    return int(frac * 2.0 ** 64)  # an exact product (a power of two), a truncating conversion


def keys(se, u, vs):
    """key(u, v) for every v of the int64 array `vs` -> a list of Python integers"""
    vs = np.asarray(vs, dtype=np.int64)
    a, b = np.minimum(vs, u).astype(np.uint64), np.maximum(vs, u).astype(np.uint64)
    return [int(k) for k in mix64(U64(se) ^ ((a << U64(32)) | b))]


def split(rowptr, colids, frac, seed=1, ratio=1):
    """-> dict(rowptr, colids, held_u, held_v, neg_u, neg_v, q: held pairs per vertex, total: negatives per vertex, and the counters)"""
    n = len(rowptr) - 1
    se, sn = seeds(seed)
    T = threshold(frac)
    nbrs = [neighbours(rowptr, colids, u) for u in range(n)]
    key = [dict(zip(nb.tolist(), keys(se, u, nb))) for u, nb in enumerate(nbrs)]
    anchor = [min(k, key=lambda v: (k[v], v)) if k else None for k in key]

    def held(u, v):  # the rule per nonzero (u, v) as written
        return u != v and key[u][v] < T and anchor[u] != v and anchor[v] != u

    out = dict(edges=0, candidates_held=0, protected=0, held=0, negatives=0, drawn=0, capped=0)
    train_rows, hu, hv, nu, nv, q, total = [], [], [], [], [], [], []
    for u in range(n):
        row = [int(v) for v in colids[rowptr[u]:rowptr[u + 1]]]
        train_rows.append([v for v in row if not held(u, v)])
        up = [v for v in nbrs[u].tolist() if v > u]
        mine = [v for v in up if held(u, v)]
        cand = sum(key[u][v] < T for v in up)
        out["edges"] += len(up)
        out["candidates_held"] += cand
        out["protected"] += cand - len(mine)
        hu += [u] * len(mine)
        hv += mine
        q.append(len(mine))
        room = (n - 1 - len(nbrs[u])) // 2
        tot = min(ratio * len(mine), room)
        out["capped"] += room < ratio * len(mine)
        taken, neg, t = set(nbrs[u].tolist()) | {u}, [], 0
        while len(neg) < tot:
            for c in candidates(sn, u, t, 64, n).tolist():
                t += 1
                if c not in taken:
                    taken.add(c)
                    neg.append(c)
                    if len(neg) == tot:
                        break
        out["drawn"] += t
        total.append(tot)
        nu += [u] * tot
        nv += neg
    out["held"], out["negatives"] = len(hu), len(nu)
    tr = np.zeros(n + 1, dtype=np.uint32)
    tr[1:] = np.cumsum([len(r) for r in train_rows])
    out["train_nnz"] = int(tr[n])
    arr = lambda x: np.array(x, dtype=np.uint32)
    out.update(rowptr=tr, colids=arr([v for r in train_rows for v in r]), held_u=arr(hu), held_v=arr(hv), neg_u=arr(nu), neg_v=arr(nv),
               q=q, total=total)
    return out


def pair_scores(X, u, v, metric):
    """float32 [m]: the similarity of rows u[i] and v[i], reported as f2v_nearest_rows reports a score (-0 as +0)"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    Q, Cc = X[np.asarray(u, dtype=np.int64)], X[np.asarray(v, dtype=np.int64)]
    acc = np.zeros(len(Q), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(X.shape[1]):
            if metric == "l2":
                t = Q[:, d] - Cc[:, d]
                acc = fma32(t, t, acc)
            else:
                acc = fma32(Q[:, d], Cc[:, d], acc)
        if metric == "l2":
            acc = -acc
        elif metric == "cos":
            acc = (acc * rnorm(Q)) * rnorm(Cc)
        return (acc + np.float32(0)).astype(np.float32)


def order_key(s):
    """The order-preserving integer of a score: larger score, larger key; -0 = +0; NaN the lowest."""
    s = float(s)
    if math.isnan(s):
        return 0
    bits = struct.unpack("<Q", struct.pack("<d", s + 0.0))[0]
    return (~bits & MASK) if bits >> 63 else bits | (1 << 63)


def ranking(scores, y):
    """-> dict(auc, ap, concordant, tied, positives, negatives, groups)"""
    y = [int(t) for t in y]
    assert all(t in (0, 1) for t in y)
    P = sum(y)
    N = len(y) - P
    assert P and N
    items = sorted(((order_key(s), t) for s, t in zip(scores, y)), key=lambda it: -it[0])
    m = len(items)
    terms = [0.0] * m
    conc = tied = groups = TP = FP = 0
    i = 0
    while i < m:
        j = i
        while j < m and items[j][0] == items[i][0]:
            j += 1
        pos = sum(t for _, t in items[i:j])
        neg = j - i - pos
        TP += pos
        FP += neg
        conc += pos * (N - FP)
        tied += pos * neg
        groups += 1
        terms[j - 1] = (float(pos) * float(TP)) / float(TP + FP)
        i = j
    total = 0.0
    for b in range(0, m, 1024):
        block = 0.0
        for t in terms[b:b + 1024]:
            block += t
        total += block
    return dict(auc=float(2 * conc + tied) / (2.0 * float(P) * float(N)), ap=total / float(P), concordant=conc, tied=tied, positives=P, negatives=N,
                groups=groups)


def pair_count(scores, y):
    """(concordant, tied) by looking at every (one, zero) pair: O(m^2)"""
    k = [order_key(s) for s in scores]
    ones = [k[i] for i in range(len(y)) if y[i] == 1]
    zeros = [k[i] for i in range(len(y)) if y[i] == 0]
    return sum(a > b for a in ones for b in zeros), sum(a == b for a in ones for b in zeros)
