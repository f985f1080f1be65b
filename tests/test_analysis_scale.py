"""The floating-point analysers where their reductions take a second pass, their gathers stride and K is 1024 (include/f2v.h:
f2v_kmeans, f2v_silhouette, f2v_davies_bouldin, f2v_nearest_rows, f2v_index_build / _build_given / _search_rows, f2v_tsne,
f2v_logreg_decision, f2v_trustworthiness).

The modules of these calls stop at n <= 9000, K <= 200, 40 lists, m <= 5000, and tests/test_analysis_values.py runs them at n = 300:
every sequential sum over parts has one pass through its staging buffer, every loop over k one trip, every gather one trip of its grid,
every chunked call one chunk.  The shapes of tests/analysis_scale.py are past those points; THRESHOLDS restates each with the constant
of the sources it is measured against and the quantity of the case that exceeds it.

Host tests: the table against the sources; the subset restatements equal the full ones on small shapes; the inputs have the properties
they are built for; every compared table says something.  -m gpu: arrays with array_equal, floats by their bits, counters with ==.  No
tolerance anywhere."""
import re

import numpy as np
import pytest

import force2vec_amd as F
from force2vec_amd import _lib
import analysis_scale as S
import analysis_values as A
import index_ref as I
import kmeans_ref as K
import layout_ref as L
import logreg_ref as LR
import nearest_ref as R
import separation_ref as SR
import tsne_ref as T
from test_kmeans import engine_for

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ENGINE, KMEANS_H, TSNE_H, LAYOUT_H, SEP_H = "f2v_engine.hip", "f2v_kmeans.hip.h", "f2v_tsne.hip.h", "f2v_layout.hip.h", "f2v_separation.hip.h"
GATHER = r"\(\(size_t\)cq \* D \+ 255\) / 256, (\d+)\)\), dim3\((\d+)\)"
DEFAULT_CHUNK = 8192  # "nearest_chunk", "index_chunk", "trust_chunk" as a handle starts (asserted on the handle by the GPU cases)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


# ---- host: which threshold every case exceeds ----------------------------------------------------------------------------------------
def gather_cap():
    """the elements one trip of nearest_gather_kernel's grid covers: workgroups x threads of its launch in nearest_run_on"""
    found = re.search(GATHER, S.source(ENGINE))
    assert found, "f2v_engine.hip no longer caps the gather's grid"
    return int(found.group(1)) * int(found.group(2))


def index_launches():
    chunk, splits = S.index_chunks(S.INDEX_NQ, S.INDEX_P, S.INDEX_K, S.INDEX_LARGEST, S.constant("kIxMaxKeys", ENGINE), S.constant("kIxManyPairs", ENGINE),
                                   tile=S.constant("kNnTile", "f2v_nearest.hip.h"), few=S.constant("kIxFewSplits", ENGINE), most=S.constant("kIxMaxSplits", ENGINE))
    return chunk, splits, -(-S.INDEX_NQ // chunk)


def thresholds():
    """(code, source, the text the source must still hold, what the case's quantity must exceed, the quantity, the case -- None: not
    reached, with the reason)"""
    c, cap = S.constant, gather_cap()
    piece, block, maxk = c("kKmPiece", KMEANS_H), c("kKmSortBlock", KMEANS_H), c("F2V_KMEANS_MAX_K")
    n1024, n258 = S.KMEANS["k1024"][0], S.KMEANS["blocks258"][0]
    chunk, splits, launches = index_launches()
    near = {name: min(n, DEFAULT_CHUNK) * D for name, (n, D, _, _) in S.NEAREST.items()}
    return [
        ("kmeans_inertia_reduce_kernel: the inertia of f2v_kmeans", KMEANS_H, "for (uint32_t p0 = 0; p0 < parts; p0 += 256)", 256, -(-n1024 // piece),
         "kmeans[k1024]"),
        ("kmeans_inertia_reduce_kernel: the score of f2v_silhouette", ENGINE, "hipLaunchKernelGGL(kmeans_inertia_reduce_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)sp.d_part",
         256, -(-S.SIL_N // c("kSepPiece", SEP_H)), "silhouette[nq16449]"),
        ("kmeans_offsets_kernel: per, lo and hi", KMEANS_H, "per = (blocks + 255) / 256", 256, -(-n258 // block), "kmeans[blocks258]"),
        ("kmeans_hist_kernel, kmeans_starts_kernel: i += blockDim.x over k", KMEANS_H, "for (uint32_t i = threadIdx.x; i < k; i += blockDim.x)", 256,
         S.KMEANS["k257"][2], "kmeans[k257]"),
        ("kmeans_hist_kernel, kmeans_starts_kernel, kmeans_scatter_kernel: the last trip over k", KMEANS_H, "for (uint32_t i = lane; i < k; i += 64)", 3 * 256,
         S.KMEANS["k1024"][2], "kmeans[k1024]"),
        ("km_tile, kmeans_piece_sum_kernel's search of pstart, kmeans_centroid_kernel's grid: K = F2V_KMEANS_MAX_K", KMEANS_H, "constexpr uint32_t kKmMaxK = 1024;",
         maxk - 1, S.KMEANS["k1024"][2], "kmeans[k1024]"),
        ("cspan, separation_finish_kernel, separation_cluster_kernel: K = F2V_SEPARATION_MAX_CLUSTERS", SEP_H, "for (uint32_t c = 0; c < f.k; c++)",
         c("F2V_SEPARATION_MAX_CLUSTERS") - 1, S.SEP_K, "separation[k1024]"),
        ("nearest_gather_kernel behind f2v_nearest_rows (and f2v_trustworthiness, which calls the same nearest_run_on)", ENGINE,
         "if (rows) hipLaunchKernelGGL(nearest_gather_kernel, dim3(std::min<size_t>(((size_t)cq * D + 255) / 256, 4096)), dim3(256), 0, c->stream, X, (const uint32_t *)w.d_qids, cq, D, w.d_Q);",
         cap, near["l2_d256"], "nearest[l2_d256]"),
        ("nearest_gather_kernel, a full chunk and a second one", ENGINE, "const uint32_t cq = std::min(w.chunk, nq - done);", cap, near["dot_d132"], "nearest[dot_d132]"),
        ("nearest_gather_kernel behind f2v_index_search_rows", ENGINE, "const uint32_t cq = std::min(chunk, nq - done), pairs = cq * P;", cap, near["dot_d132"],
         "index_search_past_one_trip_of_the_gather: the matrix of nearest[dot_d132] through four lists, all probed"),
        ("nearest_gather_kernel behind f2v_tsne_affinities", ENGINE, "hipLaunchKernelGGL(nearest_gather_kernel, dim3(std::min<size_t>(((size_t)m * D + 255) / 256, 4096))", cap,
         S.TSNE_M * S.TSNE_D, None, "m = 4166 rows of D = 8; past the cap the call would search 8229 rows of D = 132 for 3 x perplexity neighbours "
         "and calibrate them, and its P is compared to a tolerance (the device's exp), not bit for bit"),
        ("tsne_seqsum_kernel: Z and the Kullback-Leibler sum", TSNE_H, "for (uint32_t p0 = 0; p0 < count; p0 += 64)", 64, -(-S.TSNE_M // c("kTsnePiece", TSNE_H)), "tsne[d2]"),
        ("f2v_tsne: the automatic 256 rows a workgroup", ENGINE, "const uint32_t rows = w.rows ? w.rows : (m < 4096 ? 64u : 256u);", 4096 - 1, S.TSNE_M, "tsne[d2]"),
        ("f2v_logreg_decision: a second launch, z at an offset", ENGINE, "for (uint32_t lo = 0; lo < m; lo += kLrDecisionChunk)", c("kLrDecisionChunk", ENGINE), S.LOGREG_M,
         "logreg_decision"),
        ("index_search: lists = F2V_INDEX_MAX_LISTS", ENGINE, "lists = w.info.lists, P = std::min(nprobe, lists)", c("F2V_INDEX_MAX_LISTS") - 1, S.INDEX_LISTS, "index[limits]"),
        ("index_search: nprobe = F2V_INDEX_MAX_PROBES", ENGINE, "lists = w.info.lists, P = std::min(nprobe, lists)", c("F2V_INDEX_MAX_PROBES") - 1, S.INDEX_P, "index[limits]"),
        ("index_search: the automatic chunk is below \"index_chunk\"", ENGINE, "std::min<size_t>(w.chunk, kIxMaxKeys / per_query)", chunk, DEFAULT_CHUNK, "index[limits]"),
        ("index_search: more than two launches", ENGINE, "for (uint32_t done = 0; done < nq; done += chunk)", 2 * chunk, S.INDEX_NQ, "index[limits]"),
        ("index_search: kIxManyPairs switches to kIxFewSplits", ENGINE, "(uint64_t)nq * P >= kIxManyPairs ? kIxFewSplits : kIxMaxSplits", c("kIxManyPairs", ENGINE) - 1,
         S.INDEX_NQ * S.INDEX_P, "index[limits]"),
        ("f2v_trustworthiness: the upper clamp of span", ENGINE, "span = std::min(std::max(span, 256u), kTrustMaxSpan);", c("kTrustMaxSpan", LAYOUT_H),
         S.trust_span(S.TRUST_N, min(S.TRUST_NQ, DEFAULT_CHUNK)), "trustworthiness"),
    ]


def test_every_threshold_is_exceeded_or_marked_out_of_reach():
    for row in thresholds():
        code, where, text, bound, quantity, case = row[:6]
        at = S.line_of(where, text)
        assert at, "%s no longer writes: %s" % (where, text)
        print("%-60s %s:%-14s needs > %-8d has %-8d %s" % (code[:60], where, ",".join(map(str, at)), bound, quantity, case or "NOT REACHED: " + row[6]))
        if case is None:
            assert quantity <= bound and row[6]
        else:
            assert quantity > bound, (code, quantity, bound)
    # the constants the shapes were chosen against: a change of one of them must be looked at here
    c = S.constant
    assert (c("F2V_KMEANS_MAX_K"), c("F2V_SEPARATION_MAX_CLUSTERS"), c("F2V_INDEX_MAX_LISTS"), c("F2V_INDEX_MAX_PROBES"), c("F2V_NEAREST_MAX_K")) == \
        (S.KMEANS["k1024"][2], S.SEP_K, S.INDEX_LISTS, S.INDEX_P, S.INDEX_K) == (F.KMEANS_MAX_K, 1024, F.INDEX_MAX_LISTS, F.INDEX_MAX_PROBES, F.NEAREST_MAX_K)
    assert c("kKmMaxK", KMEANS_H) == c("F2V_KMEANS_MAX_K")
    assert (c("kKmSortBlock", KMEANS_H), c("kKmPiece", KMEANS_H), c("kSepPiece", SEP_H), c("kTsnePiece", TSNE_H)) == (1024, K.PIECE, SR.PIECE, T.PIECE)
    assert (c("kLrDecisionChunk", ENGINE), c("kIxMaxKeys", ENGINE), c("kIxManyPairs", ENGINE), c("kTrustMaxSpan", LAYOUT_H), gather_cap()) == \
        (262144, 1 << 24, 16384, 4096, 4096 * 256)
    # the staging widths of the two reduce kernels and the thread counts their k loops and clamps stand on
    kmeans, tsne, engine = S.source(KMEANS_H), S.source(TSNE_H), S.source(ENGINE)
    assert "__launch_bounds__(256) void kmeans_inertia_reduce_kernel" in kmeans and "__shared__ double s[256];" in kmeans
    assert "__launch_bounds__(64) void tsne_seqsum_kernel" in tsne and "__shared__ double s_p[64];" in tsne
    assert "hipLaunchKernelGGL(kmeans_hist_kernel, dim3(blocks), dim3(256)" in engine and "hipLaunchKernelGGL(kmeans_starts_kernel, dim3(1), dim3(256)" in engine
    assert "hipLaunchKernelGGL(kmeans_offsets_kernel, dim3(k), dim3(256)" in engine
    for struct in ("uint32_t splits = 0, block = 0, chunk = 8192;", "uint32_t chunk = 8192, split_tiles = 8, block = 0;", "uint32_t chunk = 8192, block = 0;"):
        assert struct in engine  # the defaults of "nearest_chunk", "index_chunk" / "index_split_tiles", "trust_chunk" / "separation_chunk"
    # the clamps of kmeans_offsets_kernel: per = 2, the last live thread and the first whose lo is `blocks`
    blocks = -(-S.KMEANS["blocks258"][0] // 1024)
    per = (blocks + 255) // 256
    assert (blocks, per) == (258, 2) and 128 * per < blocks <= 129 * per < 255 * per
    # the ragged last part, and the parts of the second pass
    assert S.KMEANS["k1024"][0] % 64 == 1 and S.SIL_N % 64 == 1 and -(-S.KMEANS["k1024"][0] // 64) - 256 == 2 and -(-S.TSNE_M // 64) - 64 == 2
    # the index: two candidate ranges of the list of 1200, 512 queries a launch, five launches
    assert index_launches() == (512, 2, 5)
    # the second chunk of the decision and of the nearest rows
    assert S.LOGREG_M - 262144 == 1030 and S.NEAREST["dot_d132"][0] - DEFAULT_CHUNK == 37
    # trustworthiness: 128 blocks of 64 samples, 16 spans wanted, 4160 candidates each before the clamp
    assert S.trust_span(S.TRUST_N, S.TRUST_NQ) == 4160 and S.trust_span(65536, S.TRUST_NQ) == 4096


def test_constants_are_read_from_the_sources():
    assert S.constant("kIxMaxKeys", ENGINE) == 16777216 and S.constant("kTsnePiece", TSNE_H) == S.constant("F2V_TSNE_PIECE") == 64
    with pytest.raises(AssertionError):
        S.constant("kNoSuchConstant", ENGINE)
    assert S.line_of(KMEANS_H, "void kmeans_inertia_reduce_kernel") and not S.line_of(KMEANS_H, "no such text")


# ---- host: the inputs -----------------------------------------------------------------------------------------------------------------
def test_inputs_have_the_properties_they_are_built_for():
    X, lab = S.separation_input()
    counts = np.bincount(lab, minlength=S.SEP_K)
    assert len(X) == len(lab) == S.SEP_N and len(counts) == S.SEP_K and counts[S.SEP_K - 1] > 0
    assert int((counts == 0).sum()) == S.SEP_EMPTY and int((counts == 1).sum()) >= S.SEP_SINGLE and counts.max() == counts[0] == S.SEP_LARGEST > SR.PIECE
    X, lab, ids = S.silhouette_input()
    assert len(ids) == len(np.unique(ids)) == S.SIL_SUBSET and {0, 16383, 16384, S.SIL_N - 1} <= set(ids.tolist()) and np.bincount(lab).min() > 4096
    X, lab, cen, q = S.index_input()
    counts = np.bincount(lab, minlength=S.INDEX_LISTS)
    assert counts.max() == counts[7] == S.INDEX_LARGEST and int((counts == 0).sum()) == S.INDEX_EMPTY and np.delete(counts, 7).max() < 16
    assert len(q) == len(np.unique(q)) == S.INDEX_NQ and cen.shape == (S.INDEX_LISTS, S.INDEX_D)
    at = S.index_ref("l2")[0]
    assert [int(((at >= lo) & (at < lo + 512)).sum()) > 0 for lo in range(0, S.INDEX_NQ, 512)] == [True] * 5  # compared queries in every launch
    rowptr, colids, values = S.tsne_P()
    dense = np.zeros((S.TSNE_M, S.TSNE_M))
    dense[np.repeat(np.arange(S.TSNE_M), np.diff(rowptr.astype(np.int64))), colids] = values
    assert np.array_equal(dense, dense.T) and abs(values.sum() - 1.0) < 1e-12 and values.min() >= T.TINY and len(values) > 2 * S.TSNE_M
    for name, (n, D, k, iters, given) in S.KMEANS.items():
        want = S.kmeans_ref(name)
        assert want.iterations == iters and not want.converged and (want.counts > 0).all(), name  # every iteration runs; no centroid is kept
    assert (S.kmeans_ref("k1024").counts < K.PIECE).all() and (S.kmeans_ref("blocks258").counts > 64 * K.PIECE).all()
    X, Y, ids = S.trust_input()
    assert len(np.unique(ids)) == S.TRUST_NQ and X.shape == (S.TRUST_N, S.TRUST_D) and Y.shape == (S.TRUST_N, S.TRUST_D2)


@pytest.mark.parametrize("name", list(S.NEAREST))
def test_nearest_rows_are_pairwise_distinct(name):
    X = S.nearest_input(name)
    assert len(np.unique(X, axis=0)) == len(X) == S.NEAREST[name][0]
    q = S.nearest_queries(len(X), X.shape[1], gather_cap())
    mid = gather_cap() // X.shape[1]
    assert len(q) == len(np.unique(q)) == 3 * S.NEAREST_SUBSET and q[0] == 0 and q[-1] == len(X) - 1 and {mid - 1, mid, mid + 1} <= set(q.tolist())


# ---- host: the subset restatements and the array forms equal the restatements -------------------------------------------------------------
@pytest.mark.parametrize("n,D,k,iters", [(300, 4, 7, 3), (700, 8, 40, 2), (64, 3, 64, 2)])
def test_array_form_of_kmeans_equals_the_restatement(n, D, k, iters):
    X = S.normal(n, n, D)
    for init in (None, X[::n // k][:k]):
        want = K.kmeans(X, k, max_iters=iters, seed=3, init=init)
        got = S.kmeans_run(X, X[K.seed_rows(n, k, 3)] if init is None else init, iters)
        assert K.same(got, want), (n, D, k, init is None)
    X = np.round(X)  # many equal rows: ties between centroids go to the lowest index in both
    assert K.same(S.kmeans_run(X, X[:k], iters), K.kmeans(X, k, max_iters=iters, init=X[:k]))


def test_array_form_of_kmeans_equals_the_restatement_at_1024_clusters():
    """The reference of `kmeans[k1024]` is kmeans_ref.kmeans: the array form that the GPU case uses returns its very bits (once, on the
    host: the restatement ranks 16449 x 1024 scores by a lexsort per row)"""
    n, D, k, iters, _ = S.KMEANS["k1024"]
    want = K.kmeans(S.kmeans_input("k1024")[0], k, max_iters=iters, seed=1)
    assert K.same(S.kmeans_ref("k1024"), want) and want.restart == 0
    assert S.kmeans_ref("k257") is S.kmeans_ref("k257") and S.kmeans_ref("k257").restart == 0  # (k257 is kmeans_ref.kmeans itself)


def test_subset_silhouette_and_its_score_equal_the_restatement():
    """Item 3 on n = 700: s(i) and `other` of a subset of the samples are those of the full call, and the full call's score is the
    piece sum of its s(i) divided by their number"""
    rng = np.random.default_rng(3)
    X, lab = S.normal(3, 700, 4), rng.integers(0, 3, 700).astype(np.uint32)
    full = SR.silhouette(X, lab)
    ids = S.spread(700, 90, (0, 63, 64, 699))
    part = SR.silhouette(X, lab, ids)
    assert same_bits(part.s, full.s[ids]) and np.array_equal(part.other, full.other[ids])
    assert same_bits(F64(S.score_of(full.s)), F64(full.score)) and S.score_of(full.s) != float(np.sum(full.s)) / 700.0


def test_subset_nearest_equals_the_restatement():
    X = S.normal(4, 500, 20)
    for metric, exclude_self in (("l2", False), ("dot", True)):
        full = R.nearest_ref(X, S.NEAREST_K, metric, qids=np.arange(500), exclude_self=exclude_self)
        q = S.nearest_queries(500, 20, 5000)
        parts = S.in_blocks(lambda lo, hi: R.nearest_ref(X, S.NEAREST_K, metric, qids=q[lo:hi], exclude_self=exclude_self), len(q), 16)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), full[0][q]) and same_bits(np.concatenate([p[1] for p in parts]), full[1][q])


def test_subset_index_search_equals_the_restatement():
    rng = np.random.default_rng(5)
    X, cen, lab = S.normal(5, 400, 8), S.normal(6, 30, 8), rng.integers(0, 28, 400).astype(np.uint32)
    q = np.sort(rng.choice(400, 150, replace=False))
    for metric in ("l2", "dot"):
        ids, sc, pr, cand = I.index_ref(X, lab, cen, 10, metric, 6, qids=q, exclude_self=True)
        at = S.spread(150, 20, (0, 149))
        part = I.index_ref(X, lab, cen, 10, metric, 6, qids=q[at], exclude_self=True)
        assert np.array_equal(part[0], ids[at]) and same_bits(part[1], sc[at]) and np.array_equal(part[2], pr[at])
        every, total = S.probes_and_candidates(X, lab, cen, q, metric, 6)
        assert np.array_equal(every, pr) and total == cand


def test_subset_trustworthiness_equals_the_restatement():
    X = S.normal(8, 400, 4)
    Y = np.ascontiguousarray(X[:, :2] + F32(0.05) * S.normal(9, 400, 2))
    ids = np.random.default_rng(8).choice(400, 100, replace=False)
    full = L.trust(X, Y, 5, ids)
    at = S.spread(100, 24, (0, 99))
    parts = S.in_blocks(lambda lo, hi: L.trust(X, Y, 5, ids[at[lo:hi]]), len(at), 8)
    assert np.array_equal(np.concatenate([p.samples_x for p in parts]), full.samples_x[at])
    assert np.array_equal(np.concatenate([p.samples_y for p in parts]), full.samples_y[at])
    assert (full.penalty_x, full.penalty_y) == (int(full.samples_x.sum()), int(full.samples_y.sum())) and full.hits > 0


# ---- host: every compared table says something ---------------------------------------------------------------------------------------------
def tables(what):
    if what in S.KMEANS:
        r = S.kmeans_ref(what)
        return [r.centroids, np.array([r.inertia]), r.counts]
    if what == "separation":
        sil, db = S.separation_ref()
        return [sil.s, np.array([sil.score, db.score]), db.scatter, db.centroids]
    if what == "silhouette":
        r = S.silhouette_ref()
        return [r.s]
    if what in S.NEAREST:
        return [S.nearest_ref(what)[2][:, 1:]]  # (the first score of an L2 query is its own zero)
    if what in ("index_l2", "index_dot"):
        return [S.index_ref(what[6:])[2]]
    if what in ("tsne2", "tsne3"):
        r = S.tsne_ref(int(what[4]))
        return [r.y, np.array([r.kl, r.z]), r.kl_values]
    if what == "logreg":
        return [S.logreg_ref()]
    _, px, py, hits = S.trust_ref()
    return [px, py, np.array([hits])]


@pytest.mark.parametrize("what", list(S.KMEANS) + ["separation", "silhouette"] + list(S.NEAREST) + ["index_l2", "index_dot", "tsne2", "tsne3", "logreg", "trust"])
def test_compared_tables_say_something(what):
    for t in tables(what):
        assert S.says_something(t), what
    if what == "separation":  # singletons score 0: 199 of the 3000 samples, not half
        sil, db = S.separation_ref()
        assert 0 < (sil.s == 0).sum() <= S.SEP_N // 10 and (sil.s < 0).any() and (sil.s > 0).any() and len(np.unique(sil.other)) > 100
    if what == "silhouette":
        r = S.silhouette_ref()
        assert (r.s < 0).sum() > 8 and (r.s > 0).sum() > 128 and len(np.unique(r.other)) == 3
    if what in ("tsne2", "tsne3"):
        r = S.tsne_ref(int(what[4]))
        assert r.kl_values[0] != r.kl_values[1] and list(r.kl_iters) == [1, 2]


# ---- GPU: k-means -----------------------------------------------------------------------------------------------------------------------
def kmeans_ok(got, want, what):
    assert np.array_equal(got.labels, want.labels) and np.array_equal(got.counts, want.counts), what
    assert same_bits(got.centroids, want.centroids), what
    assert same_bits(F64(got.inertia), F64(want.inertia)), (what, got.inertia, want.inertia)
    assert (got.iterations, bool(got.converged), got.restart) == (want.iterations, bool(want.converged), 0), what


@gpu
@pytest.mark.parametrize("name", list(S.KMEANS))
def test_kmeans_equals_the_restatement(name):
    n, D, k, iters, given = S.KMEANS[name]
    X, init = S.kmeans_input(name)
    want = S.kmeans_ref(name)
    eng = engine_for(X)
    try:
        if k == F.KMEANS_MAX_K:  # one more is refused, and the handle runs on
            with pytest.raises(F.F2VError) as e:
                eng.kmeans(k + 1, max_iters=iters, seed=1)
            assert e.value.code == _lib.F2V_EINVAL
        for _ in range(2):  # the second call reuses the workspace
            kmeans_ok(eng.kmeans(k, max_iters=iters, seed=1, init=init), want, name)
    finally:
        eng.close()


# ---- GPU: separation ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_separation_of_1024_clusters_equals_the_restatement():
    """n = 3000, K = F2V_SEPARATION_MAX_CLUSTERS: 50 empty clusters, 100 and more of one member, one of 70 (two pieces); every sample"""
    X, lab = S.separation_input()
    sil, db = S.separation_ref()
    eng = engine_for(X)
    try:
        score, s, other = eng.silhouette(lab, samples=True)
        dscore, centroids, scatter, counts = eng.davies_bouldin(lab, details=True)
    finally:
        eng.close()
    assert len(counts) == S.SEP_K and np.array_equal(counts, db.counts)
    bad = np.flatnonzero(bits(s) != bits(sil.s))
    assert same_bits(s, sil.s), ("s(i)", len(bad), int(bad[0]), s[bad[0]], sil.s[bad[0]])
    assert np.array_equal(other, sil.other) and same_bits(F64(score), F64(sil.score)), (score, sil.score)
    assert same_bits(centroids, db.centroids) and same_bits(scatter, db.scatter)
    assert same_bits(F64(dscore), F64(db.score)), (dscore, db.score)


@gpu
def test_silhouette_of_16449_samples_in_two_claims():
    """nq = n = 16384 + 64 + 1, K = 3: 258 parts of 64 samples, the last of one.  The full restatement is n^2 fma chains, so the claim is
    cut in two.  (1) s(i) and `other` of a seeded subset of 256 samples, samples 0, 16383, 16384 and 16448 among them, equal
    separation_ref.silhouette(X, labels, ids): a sample's s(i) is a function of the sample, the matrix and the labelling alone.  (2) The
    score equals kmeans_ref.piece_sum of ALL the s(i) the call returned -- sequential pieces of 64, the piece sums sequentially --
    divided by nq, bit for bit.  Together: the score is the defined sum of values of which 256 are shown right; a wrong second pass of
    the reduction fails (2) whatever the s(i) are."""
    X, lab, ids = S.silhouette_input()
    want = S.silhouette_ref()
    eng = engine_for(X)
    try:
        for _ in range(2):
            score, s, other = eng.silhouette(lab, samples=True)
            assert len(s) == S.SIL_N and same_bits(s[ids], want.s) and np.array_equal(other[ids], want.other)
            assert np.isfinite(s).all() and same_bits(F64(score), F64(S.score_of(s))), (score, S.score_of(s))
    finally:
        eng.close()


# ---- GPU: nearest rows ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(S.NEAREST))
def test_nearest_rows_past_one_trip_of_the_gather(name):
    """Every row is a query; the staged query rows behind element 4096 * 256 are written by the second trip of nearest_gather_kernel's
    grid.  192 queries against the restatement; under L2 every query must find itself first at distance +0 (the rows are pairwise
    distinct)."""
    n, D, metric, exclude_self = S.NEAREST[name]
    X = S.nearest_input(name)
    q, ids, sc = S.nearest_ref(name)
    eng = engine_for(X)
    try:
        assert eng.get_param("nearest_chunk") == eng.get_param("index_chunk") == DEFAULT_CHUNK and eng.get_param("nearest_block") == 0
        for _ in range(2):
            got = eng.nearest(k=S.NEAREST_K, metric=metric, exclude_self=exclude_self)
            assert got[0].shape == (n, S.NEAREST_K) and np.array_equal(got[0][q], ids) and same_bits(got[1][q], sc + F32(0)), name
        if metric == "l2":
            assert np.array_equal(got[0][:, 0], np.arange(n)) and same_bits(got[1][:, 0], np.zeros(n, dtype=F32))
    finally:
        eng.close()


@gpu
def test_index_search_past_one_trip_of_the_gather():
    """f2v_index_search_rows stages its query rows by a launch of nearest_gather_kernel of its own: n = 8229, D = 132, every row a query,
    8192 of them in the first launch.  Four lists, all probed: the candidates are all rows, so the 192 compared queries must return what
    nearest_ref returns for them (no call of f2v_nearest_rows stands in between), with the probe order of the restatement"""
    name = "dot_d132"
    n, D, metric, exclude_self = S.NEAREST[name]
    X = S.nearest_input(name)
    q, ids, sc = S.nearest_ref(name)
    lab = (np.arange(n) % 4).astype(np.uint32)
    probes, _ = S.probes_and_candidates(X, lab, X[:4], q, metric, 4)
    eng = engine_for(X)
    try:
        assert eng.get_param("index_chunk") == DEFAULT_CHUNK
        eng.build_index(labels=lab, centroids=X[:4])
        for _ in range(2):
            got = eng.index_search(k=S.NEAREST_K, metric=metric, nprobe=4, exclude_self=exclude_self, details=True)
            assert got[0].shape == (n, S.NEAREST_K) and np.array_equal(got[0][q], ids) and same_bits(got[1][q], sc + F32(0))
            assert np.array_equal(got[2][q], probes) and got[3]["candidates"] == n * n
    finally:
        eng.close()


# ---- GPU: the index ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_index_at_its_limits():
    """1024 lists (one of 1200 members: two candidate ranges; 40 empty), nprobe = 128, k = 128, 2100 query rows at the default
    "index_chunk": 512 queries a launch, five launches.  Probes and candidates of every query, neighbours of 128 queries spread over
    the launches."""
    X, lab, cen, q = S.index_input()
    eng = engine_for(X)
    try:
        info = eng.build_index(labels=lab, centroids=cen)
        assert (info.lists, info.largest, info.empty) == (S.INDEX_LISTS, S.INDEX_LARGEST, S.INDEX_EMPTY) and eng.get_param("index_chunk") == DEFAULT_CHUNK
        for metric in ("l2", "dot"):
            at, ids, sc, probes, candidates = S.index_ref(metric)
            got = eng.index_search(ids=q, k=S.INDEX_K, metric=metric, nprobe=S.INDEX_P, exclude_self=True, details=True)
            assert np.array_equal(got[2], probes) and got[3]["candidates"] == candidates and got[3]["nprobe"] == S.INDEX_P, metric
            assert np.array_equal(got[0][at], ids) and same_bits(got[1][at], sc + F32(0)), metric
            eng.set_param("index_chunk", 300)  # other launches, the same result
            again = eng.index_search(ids=q, k=S.INDEX_K, metric=metric, nprobe=S.INDEX_P, exclude_self=True, details=True)
            eng.set_param("index_chunk", DEFAULT_CHUNK)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:3], again[:3])) and again[3]["candidates"] == candidates
    finally:
        eng.close()


@gpu
def test_kmeans_form_of_1024_lists_is_the_clustering_call():
    X = S.index_input()[0]
    eng = engine_for(X)
    try:
        info = eng.build_index(lists=S.INDEX_LISTS, max_iters=2, seed=5)
        km = eng.kmeans(S.INDEX_LISTS, max_iters=2, seed=5, restarts=1)
        labels, cen, counts = eng.index()
        assert np.array_equal(labels, km.labels) and same_bits(cen, km.centroids) and np.array_equal(counts, km.counts)
        assert (info.lists, info.inertia, info.iterations, info.converged) == (S.INDEX_LISTS, km.inertia, km.iterations, km.converged)
        assert info.largest == int(counts.max()) and info.empty == int((counts == 0).sum())
        with pytest.raises(F.F2VError) as e:
            eng.build_index(lists=S.INDEX_LISTS + 1, max_iters=2, seed=5)
        assert e.value.code == _lib.F2V_EINVAL
    finally:
        eng.close()


# ---- GPU: t-SNE ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d2", [2, 3])
def test_tsne_of_66_pieces_equals_the_restatement(d2):
    """m = 4096 + 70: Z and the Kullback-Leibler sum add 66 piece sums, 64 and 2; "tsne_rows" stays 0, so 256 rows a workgroup.  P is
    given (a ring with chords), so nothing depends on the device's exp"""
    want = S.tsne_ref(d2)
    eng = engine_for(S.normal(S.TSNE_M, S.TSNE_M, S.TSNE_D))
    try:
        assert eng.get_param("tsne_rows") == 0
        y, info = eng.tsne(d2, iters=2, P=S.tsne_P(), init=S.tsne_start(d2), exaggeration_iters=1, kl_every=1, details=True)
    finally:
        eng.close()
    assert same_bits(y, want.y), int((bits(y) != bits(want.y)).sum())
    assert same_bits(np.array([info["kl"], info["z"]]), np.array([want.kl, want.z])), (info["kl"], want.kl, info["z"], want.z)
    assert np.array_equal(info["kl_iters"], want.kl_iters) and same_bits(info["kl_values"], want.kl_values), (info["kl_values"], want.kl_values)


# ---- GPU: the logistic decision -----------------------------------------------------------------------------------------------------------------
@gpu
def test_logreg_decision_across_its_chunk():
    X, a, b, W = S.logreg_input()
    want = S.logreg_ref()
    eng = engine_for(X)
    try:
        for _ in range(2):
            z = eng.logreg_decision(W, pairs=(a, b))
            assert z.shape == (S.LOGREG_M, S.LOGREG_CLASSES) and np.array_equal(z, want) and same_bits(z, want)
        for i in (262143, 262144, S.LOGREG_M - 1):
            one = eng.logreg_decision(W, pairs=(a[i:i + 1], b[i:i + 1]))
            assert same_bits(one[0], z[i]), i
    finally:
        eng.close()


# ---- GPU: trustworthiness -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_trustworthiness_at_the_upper_clamp_of_span():
    """n = 65536 + 300, 8192 samples in one launch: 4160 candidates a workgroup are wanted, 4096 are taken.  The penalties of 128 samples
    against the restatement; the totals are the sums of the per-sample arrays; `hits` is the number of common members of the k nearest
    rows f2v_nearest_rows returns in the two spaces (those calls have their own comparisons), and on the 128 samples the restatement's"""
    X, Y, ids = S.trust_input()
    at, px, py, hits = S.trust_ref()
    eng, flat = engine_for(X), engine_for(Y)
    try:
        assert eng.get_param("trust_chunk") == DEFAULT_CHUNK and eng.get_param("trust_block") == 0
        for _ in range(2):
            got = eng.trustworthiness(Y, k=S.TRUST_K, ids=ids, samples=True)
            assert np.array_equal(got.samples_x[at], px) and np.array_equal(got.samples_y[at], py)
            assert int(got.penalty_x) == int(got.samples_x.sum(dtype=np.uint64)) and int(got.penalty_y) == int(got.samples_y.sum(dtype=np.uint64))
        nx = eng.nearest(ids=ids, k=S.TRUST_K, metric="l2", exclude_self=True)[0]
        ny = flat.nearest(ids=ids, k=S.TRUST_K, metric="l2", exclude_self=True)[0]
    finally:
        eng.close()
        flat.close()
    common = (nx[:, :, None] == ny[:, None, :]).any(axis=2).sum(axis=1)
    assert int(got.hits) == int(common.sum()) and int(common[at].sum()) == hits
    scale = 2.0 / (float(S.TRUST_NQ) * S.TRUST_K * (2.0 * S.TRUST_N - 3.0 * S.TRUST_K - 1.0))
    assert got.trustworthiness == 1.0 - float(int(got.penalty_x)) * scale and got.continuity == 1.0 - float(int(got.penalty_y)) * scale
    assert got.overlap == float(int(got.hits)) / (float(S.TRUST_NQ) * S.TRUST_K)
