"""TEST INFRASTRUCTURE: the plain Python / numpy restatement of the "components and spanning forests" definitions of include/f2v.h,
written from the header's text: union-find components with min-id labels (and the header's synchronous hooking rounds, for the
`rounds` count alone), Kruskal in both directions over the stated order, the connected split and the induced subgraph.  Keys are
Python integers.  Nothing here knows how the kernels cut rows into pieces, reduce, hook or sort."""
import numpy as np

from heldout_ref import candidates, keys, mix64, neighbours, seeds, threshold, u64  # noqa: F401  (mix64, the key rule, the negative rule)

DROPPED = 0xFFFFFFFF
COMPONENT_COUNTERS = ("components", "isolated", "largest", "largest_label", "edges", "rounds")


def pairs(rowptr, colids):
    """the distinct pairs (a, b), a < b, that occur as a nonzero in either direction -> a sorted list"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rowptr, dtype=np.int64)))
    cols = np.asarray(colids, dtype=np.int64)
    off = rows != cols
    return sorted(set(zip(np.minimum(rows, cols)[off].tolist(), np.maximum(rows, cols)[off].tolist())))


class UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        root = x
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[x] != root:
            self.parent[x], x = root, self.parent[x]
        return root

    def union(self, a, b):
        """-> True if a and b were in two parts (now one)"""
        ra, rb = self.find(a), self.find(b)
        if ra == rb:
            return False
        self.parent[max(ra, rb)] = min(ra, rb)  # the lower id stays the root: find(v) is the part's smallest id
        return True


def hooking_rounds(n, und):
    """the header's rounds: P = L, every pair with two labels lowers P[the larger] to the smaller, L = roots under P; the last round finds nothing"""
    L = np.arange(n, dtype=np.int64)
    a, b = (np.array(x, dtype=np.int64) for x in zip(*und)) if und else (np.zeros(0, dtype=np.int64),) * 2
    rounds = 0
    while True:
        rounds += 1
        la, lb = L[a], L[b]
        cross = la != lb
        if not cross.any():
            return rounds, L
        P = L.copy()
        np.minimum.at(P, np.maximum(la, lb)[cross], np.minimum(la, lb)[cross])
        while not np.array_equal(P[P], P):
            P = P[P]
        L = P


def components(rowptr, colids):
    """-> dict(labels uint32[n], sizes uint32[n], components, isolated, largest, largest_label, edges, rounds)"""
    n = len(rowptr) - 1
    und = pairs(rowptr, colids)
    uf = UnionFind(n)
    for a, b in und:
        uf.union(a, b)
    labels = np.array([uf.find(v) for v in range(n)], dtype=np.uint32)
    count = np.bincount(labels, minlength=n)
    sizes = count[labels].astype(np.uint32)
    largest = int(count.max())
    rounds, L = hooking_rounds(n, und)
    assert np.array_equal(L, labels)
    return dict(labels=labels, sizes=sizes, components=int((count > 0).sum()), isolated=int((sizes == 1).sum()), largest=largest,
                largest_label=int(np.flatnonzero(count == largest)[0]), edges=len(und), rounds=rounds)


def bfs_labels(rowptr, colids):
    """brute force: breadth-first search from every vertex not yet seen, in ascending id"""
    n = len(rowptr) - 1
    nbr = [set() for _ in range(n)]
    for u in range(n):
        for v in colids[rowptr[u]:rowptr[u + 1]].tolist():
            if v != u:
                nbr[u].add(v)
                nbr[v].add(u)
    labels = [-1] * n
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s], front = s, [s]
        while front:
            nxt = []
            for u in front:
                for v in nbr[u]:
                    if labels[v] < 0:
                        labels[v] = s
                        nxt.append(v)
            front = nxt
    return np.array(labels, dtype=np.uint32)


def pair_keys(se, und):
    """key(a, b) of every pair -> a list of Python integers"""
    if not und:
        return []
    a, b = (np.array(x, dtype=np.uint64) for x in zip(*und))
    return [int(k) for k in mix64(np.uint64(se) ^ ((a << np.uint64(32)) | b))]


def forest(rowptr, colids, seed=1, greatest=True, bits=64):
    """Kruskal over the pairs in ascending (greatest: descending) order of (key >> (64 - bits), a, b) -> (u uint32[m], v uint32[m]), ascending by (u, v)"""
    assert 1 <= bits <= 64
    n = len(rowptr) - 1
    und = pairs(rowptr, colids)
    se, _ = seeds(seed)
    order = sorted(((k >> (64 - bits), a, b) for k, (a, b) in zip(pair_keys(se, und), und)), reverse=bool(greatest))
    uf = UnionFind(n)
    taken = sorted((a, b) for _, a, b in order if uf.union(a, b))
    return np.array([a for a, _ in taken], dtype=np.uint32), np.array([b for _, b in taken], dtype=np.uint32)


def split_connected(rowptr, colids, frac, seed=1, ratio=1, bits=64):
    """f2v_edge_split_connected -> the dict of heldout_ref.split: held iff a candidate (full key < T) and not in the greatest forest"""
    n = len(rowptr) - 1
    se, sn = seeds(seed)
    T = threshold(frac)
    fu, fv = forest(rowptr, colids, seed, True, bits)
    in_forest = set(zip(fu.tolist(), fv.tolist()))
    nbrs = [neighbours(rowptr, colids, u) for u in range(n)]
    key = [dict(zip(nb.tolist(), keys(se, u, nb))) for u, nb in enumerate(nbrs)]

    def held(u, v):
        return u != v and key[u][v] < T and (min(u, v), max(u, v)) not in in_forest

    out = dict(edges=0, candidates_held=0, protected=0, held=0, negatives=0, drawn=0, capped=0)
    train_rows, hu, hv, nu, nv = [], [], [], [], []
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
        nu += [u] * tot
        nv += neg
    out["held"], out["negatives"] = len(hu), len(nu)
    tr = np.zeros(n + 1, dtype=np.uint32)
    tr[1:] = np.cumsum([len(r) for r in train_rows])
    out["train_nnz"] = int(tr[n])
    arr = lambda x: np.array(x, dtype=np.uint32)
    out.update(rowptr=tr, colids=arr([v for r in train_rows for v in r]), held_u=arr(hu), held_v=arr(hv), neg_u=arr(nu), neg_v=arr(nv))
    return out


def subgraph(rowptr, colids, keep):
    """keep: bool[n] -> (rowptr uint32[rows + 1], colids uint32, ids uint32[rows], new_id uint32[n])"""
    keep = np.asarray(keep, dtype=bool)
    ids = np.flatnonzero(keep)
    new_id = np.full(len(keep), DROPPED, dtype=np.uint32)
    new_id[ids] = np.arange(len(ids), dtype=np.uint32)
    rows = [[int(new_id[v]) for v in colids[rowptr[u]:rowptr[u + 1]].tolist() if keep[v]] for u in ids.tolist()]
    out = np.zeros(len(ids) + 1, dtype=np.uint32)
    out[1:] = np.cumsum([len(r) for r in rows])
    return out, np.array([v for r in rows for v in r], dtype=np.uint32), ids.astype(np.uint32), new_id
