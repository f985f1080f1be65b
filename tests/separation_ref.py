"""numpy restatement of the separation definition of include/f2v.h (tests/test_separation.py, tools/): fp32 distances from the exact
fma chain of tests/nearest_ref.py and numpy's correctly rounded float32 square root, fp64 sums in pieces of 64 members and spans of
64 pieces taken in order (np.cumsum accumulates sequentially), the silhouette, its ordered mean, and the Davies-Bouldin score.
Vectorised over candidates, sequential where the definition is sequential.  Nothing here knows how the kernels tile or split."""
from collections import namedtuple

import numpy as np

import kmeans_ref as K
import nearest_ref as R

NONE = 0xFFFFFFFF
PIECE, SPAN = 64, 64
Silhouette = namedtuple("Silhouette", "score s other")
DaviesBouldin = namedtuple("DaviesBouldin", "score centroids scatter counts")


def distances(Q, X):
    """[nq, n] float32: d(q, x) = sqrtf(chain_d fma(t_d, t_d, acc)), t_d = q_d - x_d."""
    Q, X = np.ascontiguousarray(Q, dtype=np.float32), np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty((len(Q), len(X)), dtype=np.float32)
    step = max(1, 2000000 // max(len(X), 1))  # bounds the fp64 temporaries of the fma restatement
    with np.errstate(invalid="ignore"):
        for lo in range(0, len(Q), step):
            out[lo:lo + step] = np.sqrt((np.float32(0) - R.scores(Q[lo:lo + step], X, "l2")).astype(np.float32))
    return out


def ordered_sum(a):
    """a [m, ...] float32 or float64 -> the fp64 sum along axis 0 in the definition's three levels: pieces of 64 from +0, a span's
    64 piece sums from +0, the span sums from +0."""
    a = np.asarray(a, dtype=np.float64)
    pieces = np.array([K.seq_sum(a[p:p + PIECE]) for p in range(0, len(a), PIECE)])
    spans = np.array([K.seq_sum(pieces[s:s + SPAN]) for s in range(0, len(pieces), SPAN)])
    return K.seq_sum(spans)


def labelling(labels):
    """Any integer array, negative = no label -> int64 labels with -1 for 'none'."""
    lab = np.asarray(labels)
    wide = lab.astype(np.int64)
    if lab.dtype.kind == "u":
        wide = np.where(lab == NONE, -1, wide)
    return np.where(wide < 0, -1, wide)


def silhouette(X, labels, ids=None, n_clusters=None):
    X = np.ascontiguousarray(X, dtype=np.float32)
    lab = labelling(labels)
    k = int(lab.max()) + 1 if n_clusters is None else n_clusters
    ids = np.flatnonzero(lab >= 0) if ids is None else np.asarray(ids, dtype=np.int64)
    members = [np.flatnonzero(lab == c) for c in range(k)]  # ascending id
    sums = np.zeros((k, len(ids)), dtype=np.float64)
    for c in range(k):
        if len(members[c]):
            sums[c] = ordered_sum(distances(X[members[c]], X[ids]))  # [members, samples]: the squares are those of (x_i - x_j) too
    s, other = np.zeros(len(ids), dtype=np.float64), np.zeros(len(ids), dtype=np.uint32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, v in enumerate(ids):
            L = int(lab[v])
            a = sums[L, i] / float(len(members[L]) - 1) if len(members[L]) > 1 else np.nan
            b, o = None, None
            for c in range(k):
                if c == L or not len(members[c]):
                    continue
                m = sums[c, i] / float(len(members[c]))
                if b is None or m < b:
                    b, o = m, c
            mx = a if a > b else b
            s[i] = 0.0 if len(members[L]) == 1 or mx == 0.0 else (b - a) / mx
            other[i] = o
    parts = np.array([K.seq_sum(s[p:p + PIECE]) for p in range(0, len(s), PIECE)])
    return Silhouette(float(K.seq_sum(parts)) / float(len(s)), s, other)


def davies_bouldin(X, labels, n_clusters=None):
    X = np.ascontiguousarray(X, dtype=np.float32)
    lab = labelling(labels)
    k = int(lab.max()) + 1 if n_clusters is None else n_clusters
    members = [np.flatnonzero(lab == c) for c in range(k)]
    C = np.zeros((k, X.shape[1]), dtype=np.float32)
    S = np.zeros(k, dtype=np.float64)
    for c in range(k):
        if len(members[c]):
            C[c] = (K.piece_sum(X[members[c]]) / float(len(members[c]))).astype(np.float32)
            S[c] = ordered_sum(distances(X[members[c]], C[c:c + 1])[:, 0]) / float(len(members[c]))
    M = distances(C, C).astype(np.float64)
    live = [c for c in range(k) if len(members[c])]
    total = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in live:
            mx = None
            for d in live:
                if d == c:
                    continue
                ss = S[c] + S[d]
                r = 0.0 if ss == 0.0 else ss / M[c, d]
                if mx is None or r > mx:
                    mx = r
            total += mx
    counts = np.array([len(m) for m in members], dtype=np.uint64)
    return DaviesBouldin(total / float(len(live)), C, S, counts)
