"""numpy restatement of the clustering definition of include/f2v.h (tests/test_kmeans.py, tools/): the fp32 distance chain and the
k = 1 ranking of tests/nearest_ref.py, fp64 sums in pieces of 64 taken in order (np.cumsum accumulates sequentially), the iteration,
the seeded initial rows, the restarts, and the modularity tallies.  Nothing here knows how the kernels block, sort or reduce."""
from collections import namedtuple

import numpy as np

import nearest_ref as R

PIECE = 64
Result = namedtuple("Result", "labels centroids inertia iterations converged restart counts")


def mix64(z):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def seed_rows(n, k, seed):
    """The k vertices of smallest key(v) = mix64(mix64(seed) ^ v), ties by id."""
    keys = mix64(mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF)) ^ np.arange(n, dtype=np.uint64))
    return np.lexsort((np.arange(n), keys))[:k]


def assign(X, C):
    """-> (labels uint32[n], dist float32[n]): the centroid of smallest distance, ties to the lowest index, NaN last."""
    ids, sc = R.top_k(R.scores(X, C, "l2"), 1)
    return ids[:, 0].copy(), (np.float32(0) - sc[:, 0]).astype(np.float32)


def seq_sum(a):
    """Sequential fp64 sum from +0 along axis 0."""
    a = np.asarray(a, dtype=np.float64)
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1:], dtype=np.float64)


def piece_sum(a):
    """Pieces of 64 consecutive entries summed sequentially, then the piece sums summed sequentially."""
    return seq_sum(np.array([seq_sum(a[p:p + PIECE]) for p in range(0, len(a), PIECE)]))


def update(X, labels, C):
    out = C.copy()
    for c in range(C.shape[0]):
        members = np.flatnonzero(labels == c)  # ascending id
        if len(members):
            out[c] = (piece_sum(X[members]) / float(len(members))).astype(np.float32)
    return out


def inertia(dist):
    return float(piece_sum(dist))


def run(X, C0, max_iters):
    """The iteration from the centroids C0 -> Result (restart 0)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.ascontiguousarray(C0, dtype=np.float32).copy()
    prev, t = None, 1
    while True:
        labels, dist = assign(X, C)
        if t > 1 and np.array_equal(labels, prev):
            iterations, converged = t - 1, True
            break
        if t - 1 == max_iters:
            iterations, converged = max_iters, False
            break
        C = update(X, labels, C)
        prev, t = labels, t + 1
    counts = np.bincount(labels, minlength=C.shape[0]).astype(np.uint64)
    return Result(labels, C, inertia(dist), iterations, converged, 0, counts)


def kmeans(X, k, max_iters=300, seed=1, restarts=1, init=None):
    if init is not None:
        return run(X, init, max_iters)
    best = None
    for r in range(restarts):
        res = run(X, X[seed_rows(X.shape[0], k, seed + r)], max_iters)
        if best is None or res.inertia < best.inertia:
            best = res._replace(restart=r)
    return best


def same(got, want):
    """Bit for bit: labels, centroids, counts, inertia, iterations, convergence and the winning restart."""
    return (np.array_equal(got.labels, want.labels) and np.array_equal(got.centroids.view(np.uint32), want.centroids.view(np.uint32)) and
            np.array_equal(got.counts, want.counts) and got.inertia == want.inertia and got.iterations == want.iterations and
            bool(got.converged) == bool(want.converged) and got.restart == want.restart)


def tallies(rowptr, colids, labels, n_clusters):
    """(edges, inside uint64[nc], degree uint64[nc]) of the simple undirected graph of the CSR."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n), np.diff(rowptr))
    dst = np.asarray(colids, dtype=np.int64)
    pairs = np.unique(np.minimum(src, dst) * n + np.maximum(src, dst))
    u, v = pairs // n, pairs % n
    inside = np.bincount(labels[u][labels[u] == labels[v]], minlength=n_clusters)
    degree = np.bincount(labels[u], minlength=n_clusters) + np.bincount(labels[v], minlength=n_clusters)
    return len(pairs), inside.astype(np.uint64), degree.astype(np.uint64)


def modularity_q(edges, inside, degree):
    """Q = sum over c ascending of (inside[c] / m - (degree[c] / (2 m))^2) in fp64, sequentially; 0 when m = 0."""
    q, m = 0.0, float(edges)
    for i, d in zip(inside, degree):
        if edges:
            x = float(d) / (2.0 * m)
            q += float(i) / m - x * x
    return q
