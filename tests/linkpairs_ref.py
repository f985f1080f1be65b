"""TEST INFRASTRUCTURE: the numpy restatement of f2v_link_pairs (include/f2v.h: link prediction pairs), written from the header's text:
N(u), the positives, total(u) = min(ratio * p(u), A(u) / 2), the candidates c(u, t) = mix64(mix64(S1 ^ u) + t) % n accepted in order
of t, the item order and the four-round Feistel shuffle with cycle walking.  Nothing here knows how the kernels place vertices, size
their rounds or keep the accepted set."""
import numpy as np

from kmeans_ref import mix64

U64 = np.uint64


def u64(x):
    return U64(int(x) & 0xFFFFFFFFFFFFFFFF)


def shuffle_bits(M):
    b = 2
    while (1 << b) < M:
        b += 2
    return b


def perm(items, M, s2):
    """The places of the item indices `items` (all below M) under the shuffle keyed by S2 -> uint64 array."""
    half = U64(shuffle_bits(M) // 2)
    mask = U64((1 << int(half)) - 1)
    x = np.array(items, dtype=np.uint64).reshape(-1)
    todo = np.arange(len(x))
    with np.errstate(over="ignore"):
        while len(todo):
            L, R = x[todo] >> half, x[todo] & mask
            for r in range(4):
                L, R = R, L ^ (mix64(u64(s2) ^ (U64(r << 32) + R)) & mask)
            x[todo] = (L << half) | R
            todo = todo[x[todo] >= U64(M)]
    return x


def neighbours(rowptr, colids, u):
    row = np.asarray(colids[rowptr[u]:rowptr[u + 1]], dtype=np.int64)
    return np.unique(row[row != u])


def candidates(s1, u, t0, count, n):
    """c(u, t) for t = t0 .. t0 + count - 1"""
    with np.errstate(over="ignore"):
        hu = mix64(u64(s1) ^ U64(u))
        return (mix64(hu + np.arange(t0, t0 + count, dtype=np.uint64)) % U64(n)).astype(np.int64)


def pair_set(rowptr, colids, ratio=2, seed=1):
    """-> (u uint32 [M], v uint32 [M], y uint8 [M], info dict(positives, negatives, candidates, capped))"""
    n = len(rowptr) - 1
    s1 = int(mix64(u64(seed)))
    s2 = int(mix64(u64(s1)))
    us, vs, ys = [], [], []
    info = dict(positives=0, negatives=0, candidates=0, capped=0)
    for u in range(n):
        nu = neighbours(rowptr, colids, u)
        pos = nu[nu > u]
        room = (n - 1 - len(nu)) // 2
        total = min(ratio * len(pos), room)
        info["capped"] += room < ratio * len(pos)
        taken, neg, t = set(nu.tolist()) | {u}, [], 0
        while len(neg) < total:
            for c in candidates(s1, u, t, 64, n).tolist():
                t += 1
                if c not in taken:
                    taken.add(c)
                    neg.append(c)
                    if len(neg) == total:
                        break
        info["candidates"] += t
        info["positives"] += len(pos)
        info["negatives"] += total
        us += [u] * (len(pos) + total)
        vs += pos.tolist() + neg
        ys += [1] * len(pos) + [0] * total
    M = len(ys)
    place = perm(np.arange(M, dtype=np.uint64), M, s2).astype(np.int64)
    u, v, y = np.empty(M, dtype=np.uint32), np.empty(M, dtype=np.uint32), np.empty(M, dtype=np.uint8)
    u[place], v[place], y[place] = us, vs, ys
    return u, v, y, info
