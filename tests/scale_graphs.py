"""TEST INFRASTRUCTURE of tests/test_graph_scale.py: the seeded graphs on which the integer calls (link pairs, the two edge splits,
components, forests, subgraphs, Louvain, ranking) leave their first grid-stride trip and the first pass of their scans, and the
vectorised numpy / scipy references for the sizes at which the per-vertex restatements are too slow.

Every generator returns (rowptr uint32[n + 1], colids uint32[nnz]) with ascending rows, as `csr()` of tests/test_linkpairs.py does,
every edge stored in both directions.  Nothing here knows how the kernels place vertices, stride, scan or reduce."""
import functools

import numpy as np

import components_ref as CR
import heldout_ref as HR
import linkpairs_ref as LR
import louvain_ref as VR

# ---- the graphs -----------------------------------------------------------------------------------------------------------------
# total(u) at ratio 1 of the hubs of `thresholds` (= their degree: every neighbour is higher and the cap does not bind): one vertex on
# each side of 64 candidates a round, of "link_short_max" = 256 and its values 255 / 257 / 1024, and of the 3072 negatives whose table
# still fits LDS.  512 and 513: rows of exactly two pieces of 256 nonzeros, and of two and one nonzero more.
TOTALS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073)
EXTRA_ROWS = (512, 513)
THRESHOLDS_N = 9300
CAPPED_DEGREE = 4700      # the last hub: more than n / 2 neighbours, total = (n - 1 - 4700) // 2 = 2299
MEDIUM_N, MEDIUM_HUB, MEDIUM_HUB_DEGREE = 40000, 17, 2000
LARGE_N = 262144 + 1500
LARGE_CUT = 997           # edges of a stretch of the permuted path
LARGE_ISOLATED = 3000
LARGE_CHAIN = (100000, 140000)  # an ascending path over these consecutive ids
LARGE_HUB, LARGE_HUB_DEGREE = 7, 3100       # total(7) = 3100 > 3072 at ratio 1: a table in the workspace
LARGE_ROW, LARGE_ROW_DEGREE = 250000, 700   # a row of 700 nonzeros: three pieces of 256
HUGE_N = 16384 * 256 + 1000


def csr_of_pairs(n, a, b):
    """the CSR of the undirected pairs (a[i], b[i]), duplicates collapsed, both directions stored, rows ascending"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    assert (a != b).all() and a.min() >= 0 and max(a.max(), b.max()) < n
    key = np.unique(np.concatenate([a * n + b, b * n + a]))
    rows, cols = key // n, key % n
    rowptr = np.zeros(n + 1, dtype=np.uint32)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rowptr, cols.astype(np.uint32)


def hub_degrees():
    return TOTALS + EXTRA_ROWS + (CAPPED_DEGREE,)


@functools.lru_cache(maxsize=None)
def thresholds():
    """n = 9300.  Vertices 0..15 are hubs of the degrees hub_degrees(), in that order; all their neighbours are leaves (ids 16 and
    up), dealt round-robin so that a leaf has two or three hubs and nothing else."""
    n, hubs = THRESHOLDS_N, len(hub_degrees())
    leaves = n - hubs
    a, b, cursor = [], [], 0
    for h, d in enumerate(hub_degrees()):
        assert d < leaves
        a.append(np.full(d, h))
        b.append(hubs + (cursor + np.arange(d)) % leaves)
        cursor += d
    return csr_of_pairs(n, np.concatenate(a), np.concatenate(b))


@functools.lru_cache(maxsize=None)
def medium():
    """n = 40000: 80000 seeded random pairs (about four nonzeros a vertex) and vertex 17 tied to 2000 higher ids"""
    n, rng = MEDIUM_N, np.random.default_rng(40000)
    a, b = rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)
    hub = rng.choice(np.arange(MEDIUM_HUB + 1, n), MEDIUM_HUB_DEGREE, replace=False)
    a, b = np.concatenate([a, np.full(len(hub), MEDIUM_HUB)]), np.concatenate([b, hub])
    return csr_of_pairs(n, a[a != b], b[a != b])


def permuted_stretches(ids, rng, isolated, cut):
    """a path through a seeded permutation of `ids`, but for the first `isolated` of them, cut after every `cut` edges: stretches of
    cut + 1 vertices whose ids lie all over the range -> (a, b, the isolated ids)"""
    order = rng.permutation(ids)
    alone, walk = order[:isolated], order[isolated:]
    keep = np.arange(len(walk) - 1) % (cut + 1) != cut
    return walk[:-1][keep], walk[1:][keep], np.sort(alone)


@functools.lru_cache(maxsize=None)
def large_parts():
    """-> (rowptr, colids, isolated ids)"""
    n, rng = LARGE_N, np.random.default_rng(262144)
    lo, hi = LARGE_CHAIN
    chain = np.arange(lo, hi)
    a, b, alone = permuted_stretches(np.setdiff1d(np.arange(n), np.concatenate([chain, [LARGE_HUB, LARGE_ROW]])), rng, LARGE_ISOLATED, LARGE_CUT)
    hub, row = rng.choice(chain, LARGE_HUB_DEGREE, replace=False), rng.choice(chain, LARGE_ROW_DEGREE, replace=False)
    a = np.concatenate([a, chain[:-1], np.full(len(hub), LARGE_HUB), np.full(len(row), LARGE_ROW)])
    b = np.concatenate([b, chain[1:], hub, row])
    return csr_of_pairs(n, a, b) + (alone,)


def large():
    """n = 262144 + 1500.  The ids outside 100000..139999: 3000 isolated, the others in stretches of 997 edges of a path through a
    seeded permutation (many components, each spread over the whole id range).  100000..139999: one ascending path (long pointer chains
    towards the smallest id).  Vertex 7 has 3100 neighbours on that path, all higher, and vertex 250000 a row of 700 nonzeros, all
    lower."""
    return large_parts()[:2]


@functools.lru_cache(maxsize=None)
def huge():
    """n = 16384 * 256 + 1000, built like large(): stretches of 997 edges of a permuted path, 3000 isolated ids, the ascending path"""
    n, rng = HUGE_N, np.random.default_rng(16384)
    chain = np.arange(*LARGE_CHAIN)
    a, b, _ = permuted_stretches(np.setdiff1d(np.arange(n), chain), rng, LARGE_ISOLATED, LARGE_CUT)
    return csr_of_pairs(n, np.concatenate([a, chain[:-1]]), np.concatenate([b, chain[1:]]))


GRAPHS = {"thresholds": thresholds, "medium": medium, "large": large}


def graph(name):
    return GRAPHS[name]()


# ---- what the definitions give per vertex, vectorised (for the properties of the graphs and the table of caps) -----------------------
def degrees(rowptr, colids):
    """(|N(u)|, p(u)) for a CSR without duplicates and self-loops (every generator above)"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    return np.bincount(rows, minlength=n), np.bincount(rows[colids.astype(np.int64) > rows], minlength=n)


def totals(rowptr, colids, ratio):
    """total(u) = min(ratio * p(u), A(u) / 2) of f2v_link_pairs, and where the cap binds"""
    n = len(rowptr) - 1
    nu, p = degrees(rowptr, colids)
    room = (n - 1 - nu) // 2
    return np.minimum(ratio * p, room), room < ratio * p


def row_pieces(rowptr, piece=256):
    """how many pieces the rows longer than `piece` nonzeros are cut into"""
    length = np.diff(rowptr.astype(np.int64))
    return int(((length[length > piece] + piece - 1) // piece).sum())


# ---- the restatements of tests/*_ref.py on these graphs, each computed once and never modified -------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_set(name, ratio, seed=1):
    return LR.pair_set(*graph(name), ratio=ratio, seed=seed)


@functools.lru_cache(maxsize=None)
def split(name, frac, ratio, seed=1):
    return HR.split(*graph(name), frac, seed=seed, ratio=ratio)


@functools.lru_cache(maxsize=None)
def split_connected(name, frac, ratio, seed=1):
    return CR.split_connected(*graph(name), frac, seed, ratio)


@functools.lru_cache(maxsize=None)
def components(name):
    return CR.components(*graph(name))


@functools.lru_cache(maxsize=None)
def forest(name, greatest, bits=64, seed=1):
    return CR.forest(*graph(name), seed, greatest, bits)


@functools.lru_cache(maxsize=None)
def louvain(name, max_levels=32, max_sweeps=64, seed=1):
    return VR.louvain(*graph(name), seed=seed, max_levels=max_levels, max_sweeps=max_sweeps)


def keep_masks(name):
    """the two masks of the subgraph tests: ids % 3 != 0, and the largest component"""
    c = components(name)
    return {"thirds": np.arange(len(c["labels"])) % 3 != 0, "largest": c["labels"] == c["largest_label"]}


@functools.lru_cache(maxsize=None)
def subgraph(name, which):
    return CR.subgraph(*graph(name), keep_masks(name)[which])


# ---- the ranking, vectorised --------------------------------------------------------------------------------------------------------
def order_keys(scores):
    """heldout_ref.order_key of every score -> uint64: larger score, larger key; -0 = +0; NaN the lowest"""
    s = np.asarray(scores, dtype=np.float64) + 0.0
    bits = s.view(np.uint64)
    keys = np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))
    keys[np.isnan(s)] = 0
    return keys


def blocked_sum(terms, block=1024):
    """the definition's order: running sums over blocks of 1024 consecutive terms from +0, then a running sum of the block sums.
    (np.cumsum adds one after another; np.sum adds pairwise.)  The terms are not negative, so the padding zeros change nothing."""
    terms = np.asarray(terms, dtype=np.float64)
    assert len(terms) and not (terms < 0).any()
    blocks = -(-len(terms) // block)
    padded = np.zeros(blocks * block, dtype=np.float64)
    padded[:len(terms)] = terms
    return float(np.cumsum(np.cumsum(padded.reshape(blocks, block), axis=1)[:, -1])[-1])


def ranking(scores, y):
    """heldout_ref.ranking in numpy -> dict(auc, ap, concordant, tied, positives, negatives, groups), the tallies Python integers"""
    y = np.asarray(y)
    assert np.isin(y, (0, 1)).all()
    y = y.astype(np.int64)
    m, P = len(y), int(y.sum())
    N = m - P
    assert P and N and m < 2 ** 31  # every tally below m^2 < 2^62: the int64 sums cannot wrap
    keys = order_keys(scores)
    order = np.argsort(keys, kind="stable")[::-1]  # descending score
    keys, ys = keys[order], y[order]
    _, first, count = np.unique(~keys, return_index=True, return_counts=True)  # ~: ascending = the sorted order; groups of equal score
    last = first + count - 1
    ones = np.cumsum(ys)
    TP = ones[last]
    pos = np.diff(TP, prepend=0)
    neg = count - pos
    FP = last + 1 - TP
    conc, tied = int((pos * (N - FP)).sum()), int((pos * neg).sum())
    terms = np.zeros(m, dtype=np.float64)
    terms[last] = (pos.astype(np.float64) * TP.astype(np.float64)) / (TP + FP).astype(np.float64)
    return dict(auc=float(2 * conc + tied) / (2.0 * float(P) * float(N)), ap=blocked_sum(terms) / float(P), concordant=conc, tied=tied, positives=P,
                negatives=N, groups=len(first))


# ---- the components, vectorised ------------------------------------------------------------------------------------------------------
def undirected(rowptr, colids):
    """the distinct pairs (a, b), a < b, of components_ref.pairs as two int64 arrays"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rowptr, dtype=np.int64)))
    cols = np.asarray(colids, dtype=np.int64)
    key = np.unique((np.minimum(rows, cols) * n + np.maximum(rows, cols))[rows != cols])
    return key // n, key % n


def hooking_rounds(n, a, b):
    """components_ref.hooking_rounds on the arrays of the pairs -> (rounds, L)"""
    L = np.arange(n, dtype=np.int64)
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


def components_fast(rowptr, colids):
    """components_ref.components by scipy's connected_components, relabelled to the smallest id of each component"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(rowptr) - 1
    a, b = undirected(rowptr, colids)
    _, part = connected_components(csr_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(n, n)), directed=False)
    smallest = np.full(part.max() + 1, n, dtype=np.int64)
    np.minimum.at(smallest, part, np.arange(n))
    labels = smallest[part]
    count = np.bincount(labels, minlength=n)
    sizes = count[labels].astype(np.uint32)
    largest = int(count.max())
    rounds, L = hooking_rounds(n, a, b)
    assert np.array_equal(L, labels)
    return dict(labels=labels.astype(np.uint32), sizes=sizes, components=int((count > 0).sum()), isolated=int((sizes == 1).sum()), largest=largest,
                largest_label=int(np.flatnonzero(count == largest)[0]), edges=len(a), rounds=rounds)
