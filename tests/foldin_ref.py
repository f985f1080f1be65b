"""TEST INFRASTRUCTURE: the CPU restatement of f2v_fold_in (include/f2v.h: fold-in).

mix64, the negative samples and the three initial-vector rules in numpy / Python integers; one epoch of a new vertex is
`oracle.row` -- the test oracle's restatement of the step kernels' row update, ORDER_TREE and chunk 0 -- on the graph with the
vertex appended as row n: the matrix gets the vector as row n, the CSR the list as row n."""
import numpy as np

from oracle import oracle

MASK = (1 << 64) - 1
INIT_MEAN, INIT_RANDOM, INIT_GIVEN = 0, 1, 2
T_OPTIONS, SIGMOID_OPTIONS = (5, 8, 11), (6, 9)


def mix64(z):
    """the splitmix64 finaliser of include/f2v.h"""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def negatives(seed, Q, e, iters, ns, n):
    """s(Q, e, 0 .. ns-1)"""
    sm = mix64(seed)
    base = ((Q * iters + e) * ns) & MASK
    return np.array([mix64(sm ^ ((base + k) & MASK)) % n for k in range(ns)], dtype=np.uint32)


def math_of(option):
    if option in T_OPTIONS:
        return 5
    if option in SIGMOID_OPTIONS:
        return 6
    raise ValueError("option %d does not fold in" % option)


def random_vector(option, seed, Q, D):
    sm = mix64(seed)
    v = np.array([(mix64(sm ^ ((1 << 63) | ((Q * D + d) & MASK))) >> 40) for d in range(D)], dtype=np.float64) * 2.0 ** -24
    v = v.astype(np.float32)  # exact: 24-bit integers times 2^-24
    return v if math_of(option) == 6 else (np.float32(2.0) * v - np.float32(1.0)).astype(np.float32)


def mean_vector(X, ids):
    s = np.zeros(X.shape[1], dtype=np.float64)
    for j in ids:  # sequential, in list order
        s = s + X[j].astype(np.float64)
    return (s / np.float64(len(ids))).astype(np.float32)


def initial_vector(option, X, ids, kind, seed, Q, given=None):
    if kind == INIT_GIVEN:
        return np.array(given, dtype=np.float32)
    if kind == INIT_MEAN and len(ids):
        return mean_vector(X, ids)
    return random_vector(option, seed, Q, X.shape[1])


def fold_one(option, X, ids, iters, ns, lr, kind, seed, Q, given=None):
    """The vector of ONE new vertex with neighbour list `ids` whose index for every random draw is Q."""
    n, D = X.shape
    ids = np.asarray(ids, dtype=np.uint32)
    y = initial_vector(option, X, ids, kind, seed, Q, given)
    rowptr = np.zeros(n + 2, dtype=np.uint32)  # rows 0 .. n-1 are never looked at: only row n, the list
    rowptr[n + 1] = len(ids)
    colids = np.ascontiguousarray(ids if len(ids) else np.zeros(1, dtype=np.uint32))
    Xy = np.empty((n + 1, D), dtype=np.float32)
    Xy[:n] = X
    for e in range(iters):
        Xy[n] = y
        y = oracle.row(math_of(option), rowptr, colids, Xy, n, negatives(seed, Q, e, iters, ns, n), lr, order=oracle.ORDER_TREE, chunk=0)
    return y


def fold_in(option, X, lists, iters, ns, lr, kind=INIT_MEAN, seed=1, index_base=0, given=None):
    """-> float32 [len(lists), D]: f2v_fold_in restated."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty((len(lists), X.shape[1]), dtype=np.float32)
    for q, ids in enumerate(lists):
        out[q] = fold_one(option, X, ids, iters, ns, lr, kind, seed, index_base + q, None if given is None else given[q])
    return out
