"""numpy restatement of the nearest-neighbour definition of include/f2v.h (tests/test_nearest.py, tools/): exact fp32 fused
multiply-add chains over ascending d, the three similarities, and the strict total order of the ranking.  Nothing here knows
how the kernels tile, split or select."""
import numpy as np

PAD_ID = np.uint32(0xFFFFFFFF)
U = 2.0 ** -24


def fma32(a, b, c):
    """One correctly rounded fp32 fma of float32 arrays: the fp64 product of two floats is exact; the addend goes in with
    TwoSum; where the sum is inexact and its last mantissa bit even, one ulp towards the error (round to odd: 53 >= 2 * 24 + 2
    bits, so narrowing to fp32 then rounds as one rounding of the exact value would)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def chain_dot(Q, X):
    """[nq, n] float32: chain_d fma(q_d, c_d, acc) from +0."""
    acc = np.zeros((Q.shape[0], X.shape[0]), dtype=np.float32)
    for d in range(Q.shape[1]):
        acc = fma32(Q[:, d, None], X[None, :, d], acc)
    return acc


def chain_sq(V):
    acc = np.zeros(V.shape[0], dtype=np.float32)
    for d in range(V.shape[1]):
        acc = fma32(V[:, d], V[:, d], acc)
    return acc


def rnorm(V):
    n = chain_sq(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(1) / np.sqrt(n)  # numpy's float32 sqrt and divide are correctly rounded
    return np.where(n == 0, np.float32(0), r).astype(np.float32)


def scores(Q, X, metric):
    """[nq, n] float32 scores of the definition; metric 'dot' | 'l2' | 'cos'."""
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    X = np.ascontiguousarray(X, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == "l2":
            acc = np.zeros((Q.shape[0], X.shape[0]), dtype=np.float32)
            for d in range(Q.shape[1]):
                t = Q[:, d, None] - X[None, :, d]
                acc = fma32(t, t, acc)
            return -acc
        s = chain_dot(Q, X)
        if metric == "cos":
            s = (s * rnorm(Q)[:, None]) * rnorm(X)[None, :]
        return s


def top_k(S, k, excluded=None):
    """The first k candidates of every row of S in the order 'score descending, id ascending, NaN last', `excluded` (bool
    [nq, n]) left out -> (ids uint32 [nq, k], scores float32 [nq, k]), padded with 0xFFFFFFFF / -inf."""
    nq, n = S.shape
    ids = np.full((nq, k), PAD_ID, dtype=np.uint32)
    out = np.full((nq, k), -np.inf, dtype=np.float32)
    cand = np.arange(n)
    for q in range(nq):
        s = S[q]
        nan = np.isnan(s)
        order = np.lexsort((cand, np.where(nan, np.float32(0), -s), nan))
        if excluded is not None:
            order = order[~excluded[q][order]]
        order = order[:k]
        ids[q, :len(order)] = order
        out[q, :len(order)] = s[order]
    return ids, out


def exclusion_mask(qids, n, rowptr, colids, exclude_self, exclude_neighbours):
    m = np.zeros((len(qids), n), dtype=bool)
    for i, v in enumerate(qids):
        if exclude_self:
            m[i, v] = True
        if exclude_neighbours:
            m[i, colids[rowptr[v]:rowptr[v + 1]]] = True
    return m


def nearest_ref(X, k, metric, qids=None, vectors=None, rowptr=None, colids=None, exclude_self=False, exclude_neighbours=False):
    Q = X[qids] if vectors is None else vectors
    S = scores(Q, X, metric)
    mask = None
    if qids is not None and (exclude_self or exclude_neighbours):
        mask = exclusion_mask(qids, X.shape[0], rowptr, colids, exclude_self, exclude_neighbours)
    return top_k(S, k, mask)


def same(got, want):
    """Bitwise agreement of (ids, scores) pairs up to the sign of a zero score and the payload of a NaN."""
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)


def recall_counts(ids, qids, k, rowptr, colids):
    """(hits, possible) of f2v_neighbour_recall from a top-k id table computed with the query vertex excluded."""
    hits = possible = 0
    for i, v in enumerate(qids):
        nb = np.unique(colids[rowptr[v]:rowptr[v + 1]])
        nb = nb[nb != v]
        hits += int(np.isin(ids[i][ids[i] != PAD_ID], nb).sum())
        possible += min(k, len(nb))
    return hits, possible
