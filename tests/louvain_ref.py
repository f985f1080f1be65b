"""The communities of include/f2v.h (section "communities") restated with Python integers, and the agreement of two labellings.

louvain(rowptr, colids, seed, max_levels, max_sweeps) -> dict(labels, level_labels, records, communities, levels, edges, two_m,
degrees); agreement(a, b) -> dict of the integers and the fp64 scores.  Written from the header's text, not from the kernels."""
import numpy as np

from exact_ref import flog
from kmeans_ref import mix64

PHASES = 8
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1


def level0(rowptr, colids):
    """the simple graph of the CSR: per vertex {neighbour: 1} without itself, loop (0 | 1)"""
    n = len(rowptr) - 1
    adj, loop = [], []
    for u in range(n):
        row = set(int(v) for v in colids[rowptr[u]:rowptr[u + 1]])
        loop.append(1 if u in row else 0)
        row.discard(u)
        adj.append({v: 1 for v in row})
    return adj, loop


def symmetric(adj):
    return all(u in adj[v] for u in range(len(adj)) for v in adj[u])


def qnum(adj, loop, c, tot, two_m):
    inside = 2 * sum(loop)
    for i, row in enumerate(adj):
        ci = c[i]
        inside += sum(w for j, w in row.items() if c[j] == ci)
    return inside * two_m - sum(t * t for t in tot)


def run_level(adj, loop, k, two_m, seed, level, max_sweeps):
    """-> kept labelling, sweeps, moves, best, start"""
    N = len(adj)
    c, tot, size = list(range(N)), list(k), [1] * N
    sl = mix64((seed + level) & M64)
    cls = [mix64(sl ^ i) % PHASES for i in range(N)]
    start = qnum(adj, loop, c, tot, two_m)
    best, kept, sweeps, moves = start, list(c), 0, 0
    while sweeps < max_sweeps:
        for p in range(PHASES):
            decided = []
            for i in range(N):
                if cls[i] != p or not adj[i]:
                    continue
                a, ki = c[i], k[i]
                e = {}
                for j, w in adj[i].items():
                    e[c[j]] = e.get(c[j], 0) + w
                score = lambda d: e.get(d, 0) * two_m - ki * (tot[d] - ki if d == a else tot[d])
                b = min(e, key=lambda d: (-score(d), d))
                if b == a or not score(b) > score(a):
                    continue
                if size[a] == 1 and size[b] == 1 and b > a:
                    continue
                decided.append((i, b))
            for i, b in decided:
                a = c[i]
                tot[a] -= k[i]
                tot[b] += k[i]
                size[a] -= 1
                size[b] += 1
                c[i] = b
            moves += len(decided)
        sweeps += 1
        q = qnum(adj, loop, c, tot, two_m)
        if q > best:
            best, kept = q, list(c)
        else:
            break
    return kept, sweeps, moves, best, start


def aggregate(adj, loop, kept):
    ids = sorted(set(kept))
    new = {cid: r for r, cid in enumerate(ids)}
    K = len(ids)
    nadj, nloop = [dict() for _ in range(K)], [0] * K
    inside2 = [0] * K
    for i, row in enumerate(adj):
        C = new[kept[i]]
        nloop[C] += loop[i]
        for j, w in row.items():
            D = new[kept[j]]
            if D == C:
                inside2[C] += w  # ordered pairs: every unordered pair twice
            else:
                nadj[C][D] = nadj[C].get(D, 0) + w
    for C in range(K):
        nloop[C] += inside2[C] // 2
    return nadj, nloop, [new[x] for x in kept]


def louvain(rowptr, colids, seed=1, max_levels=32, max_sweeps=64):
    rowptr, colids = np.asarray(rowptr), np.asarray(colids)
    n = len(rowptr) - 1
    adj, loop = level0(rowptr, colids)
    if not symmetric(adj):
        raise ValueError("the CSR is not structurally symmetric")
    degrees = [len(adj[u]) + 2 * loop[u] for u in range(n)]
    two_m = sum(degrees)
    if two_m >= 2 ** 31:
        raise ValueError("2m is not below 2^31")
    labels = list(range(n))
    level_labels, records = [], []
    for level in range(max_levels):
        k = [sum(adj[i].values()) + 2 * loop[i] for i in range(len(adj))]
        kept, sweeps, moves, best, start = run_level(adj, loop, k, two_m, seed, level, max_sweeps)
        nodes = len(adj)
        adj, loop, renumbered = aggregate(adj, loop, kept)
        labels = [renumbered[x] for x in labels]
        level_labels.append(list(labels))
        records.append(dict(nodes=nodes, communities=len(adj), sweeps=sweeps, moves=moves, qnum=best, start=start))
        if best == start:
            break
    return dict(labels=np.array(labels, dtype=np.uint32), level_labels=np.array(level_labels, dtype=np.uint32).reshape(len(records), n),
                records=records, communities=len(adj), levels=len(records), edges=two_m // 2, two_m=two_m, degrees=degrees)


def modularity(rowptr, colids, labels):
    """Q of a labelling on the simple graph of the CSR, in exact rational arithmetic rounded once (for comparisons with a margin)"""
    adj, loop = level0(np.asarray(rowptr), np.asarray(colids))
    two_m = sum(len(a) + 2 * l for a, l in zip(adj, loop))
    K = int(max(labels)) + 1 if len(labels) else 0
    tot = [0] * K
    for u, a in enumerate(adj):
        tot[labels[u]] += len(a) + 2 * loop[u]
    if two_m == 0:
        return 0.0
    return qnum(adj, loop, [int(x) for x in labels], tot, two_m) / float(two_m * two_m)


# ---- the agreement of two labellings ---------------------------------------------------------------------------------------------
def _pieced(cells):
    """sum of n * flog(n) over the nonzero cells, in order: pieces of 1024 consecutive cells from +0, the piece sums in order"""
    cells = np.asarray(cells, dtype=np.int64).ravel()
    total = 0.0
    for lo in range(0, len(cells), 1024):
        piece = cells[lo:lo + 1024]
        nz = piece[piece > 0].astype(np.float64)
        terms = nz * flog(nz)
        s = 0.0
        for t in terms:
            s = s + float(t)
        total = total + s
    return total


def _log(x):
    return float(flog(np.array([float(x)]))[0])


def agreement(a, ka, b, kb):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    both = (a != NONE) & (b != NONE) & (a >= 0) & (b >= 0)
    table = np.zeros((ka, kb), dtype=np.int64)
    np.add.at(table, (a[both], b[both]), 1)
    rows, cols = table.sum(axis=1), table.sum(axis=0)
    N = int(both.sum())
    comb = lambda x: int((x * (x - 1) // 2).sum())
    out = dict(n=N, sum_comb=comb(table), sum_a=comb(rows), sum_b=comb(cols), total=N * (N - 1) // 2,
               rows=int((rows > 0).sum()), cols=int((cols > 0).sum()))
    S_ab, S_a, S_b = _pieced(table), _pieced(rows), _pieced(cols)
    Nf = float(N)
    logN = _log(N)
    one_a, one_b = out["rows"] == 1, out["cols"] == 1  # a side with one non-empty class: no entropy, no shared information
    Ha, Hb = 0.0 if one_a else logN - S_a / Nf, 0.0 if one_b else logN - S_b / Nf
    mi = 0.0 if one_a or one_b else max(0.0, (S_ab - S_a - S_b) / Nf + logN)
    out["entropy_a"], out["entropy_b"], out["mi"] = Ha, Hb, mi
    out["nmi"] = 1.0 if Ha == 0.0 and Hb == 0.0 else mi / (0.5 * (Ha + Hb))
    sc, sa, sb, tt = float(out["sum_comb"]), float(out["sum_a"]), float(out["sum_b"]), float(out["total"])
    den = 0.5 * (sa + sb) - sa * sb / tt
    out["ari"] = 1.0 if den == 0.0 else (sc - sa * sb / tt) / den
    return out
