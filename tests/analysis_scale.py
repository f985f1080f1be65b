"""TEST INFRASTRUCTURE of tests/test_analysis_scale.py: the seeded shapes at which the floating-point analysers (k-means, silhouette
and Davies-Bouldin, nearest rows, the index, t-SNE, the logistic decision, trustworthiness) leave the first trip of their reductions
and gathers and reach K = 1024, the constants of the sources those shapes are measured against, and the restatements of tests/*_ref.py
on them, each computed once and never modified.

Where a full restatement is n^2 fma chains the claim is cut to a subset of the samples (`spread`, the SUBSET constants); the subset
restatements are the same functions of tests/*_ref.py given fewer queries, and tests/test_analysis_scale.py shows on small shapes that
they equal the full ones.  `assign` / `kmeans_run` restate kmeans_ref.assign / .run with numpy's argmax in place of a lexsort per row (the
same order where no score is a NaN), for n = 263173 and K = 1024; shown equal to kmeans_ref.kmeans on small shapes and on `k1024` itself.  Nothing here knows how the
kernels tile, stage, stride or reduce: the thresholds below are read from the sources, the shapes are numbers."""
import functools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import analysis_values as A
import index_ref as I
import kmeans_ref as K
import layout_ref as L
import logreg_ref as LR
import nearest_ref as R
import separation_ref as SR
import tsne_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "force2vec_amd", "csrc")
F32, F64 = np.float32, np.float64

# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
KMEANS = {  # name -> (n, D, K, iterations, init given)
    "k1024": (16384 + 64 + 1, 4, 1024, 2, False),   # 258 inertia parts, the last of one distance; every k loop on its fourth trip
    "k257": (3000, 8, 257, 3, False),               # the k loops on their second trip, by one cluster
    "blocks258": (262144 + 1024 + 5, 4, 3, 2, True),  # 258 sort blocks: per = 2, the threads from 129 on start at `blocks`
}
SEP_N, SEP_D, SEP_K, SEP_LARGEST, SEP_SINGLE, SEP_EMPTY = 3000, 8, 1024, 70, 100, 50
SIL_N, SIL_D, SIL_K, SIL_SUBSET = 16384 + 64 + 1, 4, 3, 256
NEAREST = {  # name -> (n, D, metric, exclude_self)
    "l2_d256": (4200, 256, "l2", False),        # one chunk of 4200 * 256 = 1075200 elements; D > 128: the 32-query form
    "dot_d132": (8192 + 37, 132, "dot", True),  # a chunk of 8192 * 132 = 1081344 elements and one of 37 queries
}
NEAREST_K, NEAREST_SUBSET = 5, 64               # 64 queries at the start, 64 around element 2^20 / D, the last 64
INDEX_N, INDEX_D, INDEX_LISTS, INDEX_LARGEST, INDEX_EMPTY, INDEX_NQ, INDEX_P, INDEX_K, INDEX_SUBSET = 5000, 8, 1024, 1200, 40, 2100, 128, 128, 128
TSNE_M, TSNE_D = 4096 + 70, 8
LOGREG_N, LOGREG_D, LOGREG_M, LOGREG_CLASSES = 600, 4, 262144 + 1030, 2
TRUST_N, TRUST_D, TRUST_D2, TRUST_K, TRUST_NQ, TRUST_SUBSET = 65536 + 300, 4, 2, 5, 8192, 128


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def normal(seed, n, D):
    return frozen(np.random.default_rng(seed).standard_normal((n, D)).astype(F32))


def spread(nq, count, must=()):
    """`count` ascending positions below nq: `must` and seeded others"""
    rest = np.setdiff1d(np.arange(nq), np.array(must, dtype=np.int64))
    pick = np.random.default_rng(nq).choice(rest, count - len(must), replace=False)
    return np.sort(np.concatenate([np.array(must, dtype=np.int64), pick]))


def in_blocks(f, count, block):
    """[f(lo, hi) for the blocks of `block` consecutive items of `count`], eight blocks at a time: the fma chains of nearest_ref are
    numpy passes over temporaries, which run side by side and stay in cache when a block is small.  Every item's result is a function
    of the item alone, so the blocks change nothing"""
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda lo: f(lo, min(lo + block, count)), range(0, count, block)))


# ---- the constants of the sources -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source(name):
    return open(os.path.join(ROOT, "include", name) if name.endswith("f2v.h") else os.path.join(CSRC, name)).read()


def constant(name, where="f2v.h"):
    """the value of `#define name` in include/f2v.h or of the `constexpr ... name = ...;` line of a kernel source.  A tripwire, not a
    parser: it reads integers, `<<`, `*`, `+`, brackets, a `u` suffix, the casts (size_t) / (uint32_t) / (uint64_t) and one F2V_ name.
    A definition written any other way fails the assertion below with (name, the text it found) and is to be looked at by hand"""
    text = source(where)
    found = re.search(r"^#define %s ([^/\n]+)" % name, text, re.M) or re.search(r"^constexpr \w+ %s = ([^;]+);" % name, text, re.M)
    assert found, "%s no longer defines %s" % (where, name)
    value = re.sub(r"\((size_t|uint32_t|uint64_t)\)", "", found.group(1)).strip()
    if re.fullmatch(r"F2V_\w+", value):
        return constant(value)
    assert re.fullmatch(r"[0-9 <*+()u]+", value), (name, value)
    return int(eval(value.replace("u", ""), {"__builtins__": {}}))


def line_of(where, text):
    """the 1-based numbers of the lines of a source that hold `text`"""
    return [i + 1 for i, line in enumerate(source(where).split("\n")) if text in line]


# ---- k-means ------------------------------------------------------------------------------------------------------------------------
def assign(X, C):
    """kmeans_ref.assign for rows without a NaN: the same fma chains, the first centroid of largest score by numpy's argmax (ties to
    the lowest index, as the lexsort of nearest_ref.top_k orders them), in blocks of rows that bound the temporaries"""
    def block(lo, hi):
        S = R.scores(X[lo:hi], C, "l2")
        assert not np.isnan(S).any()
        best = np.argmax(S, axis=1)
        return best.astype(np.uint32), (F32(0) - S[np.arange(len(S)), best]).astype(F32)
    parts = in_blocks(block, len(X), max(1, 65536 // len(C)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def kmeans_run(X, C0, max_iters):
    """kmeans_ref.run with `assign` above"""
    X = np.ascontiguousarray(X, dtype=F32)
    C = np.ascontiguousarray(C0, dtype=F32).copy()
    prev, t = None, 1
    while True:
        labels, dist = assign(X, C)
        if t > 1 and np.array_equal(labels, prev):
            iterations, converged = t - 1, True
            break
        if t - 1 == max_iters:
            iterations, converged = max_iters, False
            break
        C = K.update(X, labels, C)
        prev, t = labels, t + 1
    counts = np.bincount(labels, minlength=C.shape[0]).astype(np.uint64)
    return K.Result(labels, C, K.inertia(dist), iterations, converged, 0, counts)


@functools.lru_cache(maxsize=None)
def kmeans_input(name):
    """-> (X, init or None).  `blocks258`: three centres that overlap and a start beside them: no cluster empties, labels move for many iterations"""
    n, D, k, _, given = KMEANS[name]
    rng = np.random.default_rng(n + k)
    if not given:
        return normal(n + k, n, D), None
    centres = rng.standard_normal((k, D))
    X = (centres[rng.integers(0, k, n)] + rng.standard_normal((n, D))).astype(F32)
    return frozen(X), frozen((centres + rng.standard_normal((k, D))).astype(F32))


@functools.lru_cache(maxsize=None)
def kmeans_ref(name, seed=1):
    """`k257`: kmeans_ref.kmeans itself.  `k1024` and `blocks258`: `kmeans_run` (a lexsort per row and centroid table takes 12 s and
    minutes there); tests/test_analysis_scale.py shows `k1024` equal to kmeans_ref.kmeans once on the host"""
    n, D, k, iters, given = KMEANS[name]
    X, init = kmeans_input(name)
    if name == "k257":
        return K.kmeans(X, k, max_iters=iters, seed=seed)
    return kmeans_run(X, init if given else X[K.seed_rows(n, k, seed)], iters)


# ---- separation ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def separation_input():
    """n = 3000, K = 1024: cluster 0 has 70 members, 1 .. 100 are singletons, 101 .. 150 stay empty, the others share the rest (cluster
    1023 among them); which vertex has which label is a seeded permutation"""
    rng = np.random.default_rng(SEP_K)
    others = np.arange(1 + SEP_SINGLE + SEP_EMPTY, SEP_K)
    rest = SEP_N - SEP_LARGEST - SEP_SINGLE
    lab = np.concatenate([np.zeros(SEP_LARGEST, dtype=np.int64), np.arange(1, 1 + SEP_SINGLE), others, rng.choice(others, rest - len(others))])
    return normal(SEP_N, SEP_N, SEP_D), frozen(rng.permutation(lab).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def separation_ref():
    X, lab = separation_input()
    return SR.silhouette(X, lab, n_clusters=SEP_K), SR.davies_bouldin(X, lab, n_clusters=SEP_K)


@functools.lru_cache(maxsize=None)
def silhouette_input():
    """n = nq = 16449, K = 3: three centres two apart, so that s(i) has both signs"""
    rng = np.random.default_rng(SIL_N)
    lab = rng.integers(0, SIL_K, SIL_N)
    X = (2.0 * rng.standard_normal((SIL_K, SIL_D))[lab] + rng.standard_normal((SIL_N, SIL_D))).astype(F32)
    lab[rng.integers(0, SIL_N, SIL_N // 10)] = rng.integers(0, SIL_K, SIL_N // 10)  # a tenth of the labels drawn again: some s(i) < 0
    return frozen(X), frozen(lab.astype(np.uint32)), frozen(spread(SIL_N, SIL_SUBSET, (0, 16383, 16384, SIL_N - 1)))


@functools.lru_cache(maxsize=None)
def silhouette_ref():
    X, lab, ids = silhouette_input()
    return SR.silhouette(X, lab, ids, n_clusters=SIL_K)


def score_of(s):
    """the silhouette score from the samples' s(i): sequential pieces of 64, the piece sums sequentially, divided by their number"""
    return float(K.piece_sum(np.asarray(s, dtype=F64))) / float(len(s))


# ---- nearest rows ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nearest_input(name):
    n, D, _, _ = NEAREST[name]
    return normal(n + D, n, D)


def nearest_queries(n, D, gather_cap):
    """the first 64 rows, the 64 around the query that holds element `gather_cap` of the staged rows, the last 64"""
    mid = gather_cap // D
    return np.concatenate([np.arange(NEAREST_SUBSET), np.arange(mid - NEAREST_SUBSET // 2, mid + NEAREST_SUBSET // 2), np.arange(n - NEAREST_SUBSET, n)])


@functools.lru_cache(maxsize=None)
def nearest_ref(name, gather_cap=1 << 20):
    n, D, metric, exclude_self = NEAREST[name]
    q = nearest_queries(n, D, gather_cap)
    parts = in_blocks(lambda lo, hi: R.nearest_ref(nearest_input(name), NEAREST_K, metric, qids=q[lo:hi], exclude_self=exclude_self), len(q), 16)
    return q, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ---- the index ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def index_input():
    """-> (X, labels, centroids, query rows).  List 7 has 1200 members, lists 100 .. 139 are empty, the others share the rest (one to
    twelve members each); the centroids are seeded rows of their own, not the lists' means: an index the caller gives"""
    rng = np.random.default_rng(INDEX_LISTS)
    others = np.setdiff1d(np.arange(INDEX_LISTS), np.concatenate([[7], np.arange(100, 100 + INDEX_EMPTY)]))
    lab = np.concatenate([np.full(INDEX_LARGEST, 7), others, rng.choice(others, INDEX_N - INDEX_LARGEST - len(others))])
    q = np.sort(rng.choice(INDEX_N, INDEX_NQ, replace=False)).astype(np.uint32)
    return normal(INDEX_N, INDEX_N, INDEX_D), frozen(rng.permutation(lab).astype(np.uint32)), normal(INDEX_LISTS + 1, INDEX_LISTS, INDEX_D), frozen(q)


def probes_and_candidates(X, labels, centroids, qids, metric, nprobe):
    """What index_ref returns beside the neighbours, for every query: the probed lists in the defined order, and the members of the probed
    lists summed over the queries"""
    pr = R.top_k(R.scores(X[qids], centroids, metric), min(nprobe, len(centroids)))[0]
    counts = np.bincount(labels, minlength=len(centroids))
    return pr, int(counts[pr].sum())


@functools.lru_cache(maxsize=None)
def index_ref(metric):
    """-> (positions of the compared queries, ids, scores, probes of ALL queries, candidates of ALL queries)"""
    X, lab, cen, q = index_input()
    at = spread(INDEX_NQ, INDEX_SUBSET, (0, INDEX_NQ - 1))
    ids, sc, pr, _ = I.index_ref(X, lab, cen, INDEX_K, metric, INDEX_P, qids=q[at], exclude_self=True)
    every, candidates = probes_and_candidates(X, lab, cen, q, metric, INDEX_P)
    assert np.array_equal(every[at], pr)
    return at, ids, sc, every, candidates


def index_chunks(nq, P, k, largest, max_keys, many_pairs, tile=128, split_tiles=8, few=2, most=16, chunk=8192):
    """the queries per launch and the candidate ranges of index_search as f2v_engine.hip derives them (defaults: the handle's)"""
    tiles = -(-largest // tile)
    cap = few if nq * P >= many_pairs else most
    tps = split_tiles
    splits = max(1, -(-tiles // tps))
    if splits > cap:
        tps = -(-tiles // cap)
        splits = -(-tiles // tps)
    return max(1, min(chunk, max_keys // (P * splits * k))), splits


# ---- t-SNE ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tsne_P():
    """A symmetric sparse P on the ring with chords of analysis_values.graph: seeded weights in 0.5 .. 1.5, the same both ways, summing to 1"""
    rowptr, colids = A.graph(TSNE_M)
    rows = np.repeat(np.arange(TSNE_M), np.diff(rowptr.astype(np.int64)))
    cols = colids.astype(np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    w = 0.5 + (K.mix64(lo.astype(np.uint64) * np.uint64(TSNE_M) + hi.astype(np.uint64)) >> np.uint64(11)).astype(F64) / 2.0 ** 53
    return rowptr, colids, frozen(w / w.sum())


def tsne_start(d2):
    return 1e-4 * np.random.default_rng(TSNE_M + d2).standard_normal((TSNE_M, d2))


@functools.lru_cache(maxsize=None)
def tsne_ref(d2):
    return T.run(tsne_P(), tsne_start(d2), iters=2, exaggeration_iters=1, kl_every=1, exact=True)


# ---- the logistic decision ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logreg_input():
    """-> (X [600, 4], a, b, W [2, 5])"""
    rng = np.random.default_rng(LOGREG_M)
    a, b = rng.integers(0, LOGREG_N, LOGREG_M).astype(np.uint32), rng.integers(0, LOGREG_N, LOGREG_M).astype(np.uint32)
    return normal(LOGREG_N, LOGREG_N, LOGREG_D), frozen(a), frozen(b), frozen(rng.standard_normal((LOGREG_CLASSES, LOGREG_D + 1)))


@functools.lru_cache(maxsize=None)
def logreg_ref():
    X, a, b, W = logreg_input()
    return frozen(LR.logits(LR.features(X, a, b, LR.HADAMARD), W))


# ---- trustworthiness ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trust_input():
    """-> (X [n, 4], Y [n, 2]: two columns of X plus noise, so that some neighbourhoods survive and some do not; 8192 seeded samples)"""
    rng = np.random.default_rng(TRUST_N)
    X = rng.standard_normal((TRUST_N, TRUST_D)).astype(F32)
    Y = (X[:, :TRUST_D2] + F32(0.05) * rng.standard_normal((TRUST_N, TRUST_D2)).astype(F32)).astype(F32)
    ids = rng.choice(TRUST_N, TRUST_NQ, replace=False).astype(np.uint32)
    return frozen(X), frozen(np.ascontiguousarray(Y)), frozen(ids)


@functools.lru_cache(maxsize=None)
def trust_ref():
    """-> (positions of the compared samples, their penalties samples_x, samples_y of layout_ref.trust, their common neighbours)"""
    X, Y, ids = trust_input()
    at = spread(TRUST_NQ, TRUST_SUBSET, (0, TRUST_NQ - 1))
    parts = in_blocks(lambda lo, hi: L.trust(X, Y, TRUST_K, ids[at[lo:hi]].astype(np.int64)), len(at), 8)
    return at, np.concatenate([p.samples_x for p in parts]), np.concatenate([p.samples_y for p in parts]), sum(p.hits for p in parts)


def trust_span(n, cq, block=64):
    """candidates per workgroup of the ranking before the two clamps, as f2v_engine.hip derives it from n and the samples of a launch"""
    want = max(1, 2048 // -(-cq // block))
    return -(-(-(-n // want)) // 64) * 64


def says_something(table):
    """at least half of a compared table is finite and not zero"""
    t = np.asarray(table, dtype=F64)
    return bool((np.isfinite(t) & (t != 0)).mean() >= 0.5)
