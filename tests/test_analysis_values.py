"""The floating-point analysers -- nearest neighbours, the index, k-means, silhouette and Davies-Bouldin, PCA, trustworthiness, the
t-SNE iteration, the logistic-regression features -- at zero, inf, NaN, huge and subnormal values (tests/analysis_values.py: the
inputs and the hand-derived rules; DESIGN.md "Special values in the analysers").

Host tests (no GPU): the restatements' results on these inputs say something (most scores finite, subnormal scores, -0 / +0 ties, NaN
and inf where planted, ...), and the restatements obey the rules of include/f2v.h as analysis_values states them by hand, pair of
classes by pair of classes -- so that a GPU comparison cannot pass because kernel and restatement share one mistake.
-m gpu: every call against its restatement on those inputs.  Every comparison is identical bits with a NaN where a NaN is expected
(extreme_values.same_values; analysis_values.same_bits for fp64 results), or nearest_ref.same plus "no zero with a sign bit" where the
header reports -0 as +0.  The one tolerance is test_logreg.close_enough for the logistic loss and gradient (device exp / log1p)."""
import functools

import numpy as np
import pytest

import force2vec_amd as F
import analysis_values as A
import extreme_values as E
import index_ref
import kmeans_ref as K
import layout_ref as L
import logreg_ref as LR
import nearest_ref as R
import separation_ref as S
import tsne_ref as T
from analysis_values import NotSpecial
from test_logreg import close_enough

gpu = pytest.mark.gpu
N, DIMS, METRICS = A.N, A.DIMS, A.METRICS
F32, F64 = np.float32, np.float64
KS = (1, 10, 128)
MD = [(name, D) for name in A.MATRICES for D in DIMS]
SEP_CASES = ([("a", name, D) for name in ("finite", "tiny", "huge") for D in (16, 128)] +
             [(which, name, D) for which in ("b", "c") for name in ("finite", "nonfinite") for D in (16, 128)] + [("d", "finite", 16), ("d", "finite", 128)])
FEATURES = ("hadamard", "l1", "l2", "average", None)  # None: the rows form


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the restatements' side, computed once -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_scores(name, D, metric, vectors=False):
    """[nq, n] scores of the restatement: every row (or every vector query) against every row."""
    X = A.matrix(name, D)[0]
    return frozen(R.scores(A.vector_queries(D) if vectors else X, X, metric))


def queries_of(name, D, form):
    return np.arange(N, dtype=np.uint32) if form == "all" else A.few_queries(A.matrix("nonfinite", D)[1])


@functools.lru_cache(maxsize=None)
def ref_rows(name, D, metric, flags, form):
    """The restatement's first 128 of every query row (a shorter result is its prefix: top_k cuts one order)."""
    q = queries_of(name, D, form)
    mask = R.exclusion_mask(q, N, *A.graph(), bool(flags & 1), bool(flags & 2)) if flags else None
    return frozen(*R.top_k(ref_scores(name, D, metric)[q], 128, mask))


@functools.lru_cache(maxsize=None)
def ref_vectors(name, D, metric):
    return frozen(*R.top_k(ref_scores(name, D, metric, True), 128))


def silhouette_case(which, name, D):
    """-> (X, labels, classes) of a separation case"""
    if which == "d":
        X, lab, _ = A.coincident_case(D)
        return X, lab, A.matrix("finite", D)[1]
    X, classes = A.matrix(name, D)
    return X, A.labelling(which, A.matrix("nonfinite", D)[1]), classes


@functools.lru_cache(maxsize=None)
def ref_separation(which, name, D):
    X, lab, _ = silhouette_case(which, name, D)
    return S.silhouette(X, lab), S.davies_bouldin(X, lab)


@functools.lru_cache(maxsize=None)
def silhouette_parts(which, name, D):
    """a(i) [n] and the other clusters' means [n, k] (NaN column for the own cluster) from the restatement's distances and sums."""
    X, lab, _ = silhouette_case(which, name, D)
    k = int(lab.max()) + 1
    means, a = np.full((N, k), np.nan), np.full(N, np.nan)
    with np.errstate(all="ignore"):
        for c in range(k):
            members = np.flatnonzero(lab == c)
            total = S.ordered_sum(S.distances(X[members], X))
            means[:, c] = total / float(len(members))
            own = lab == c
            a[own] = total[own] / float(len(members) - 1) if len(members) > 1 else np.nan
    return a, means


@functools.lru_cache(maxsize=None)
def ref_pca(name, D):
    return L.pca(A.matrix(name, D)[0], 2)


@functools.lru_cache(maxsize=None)
def ref_kmeans(name, D, iters=6):
    X = A.matrix(name, D)[0]
    return K.kmeans(X, 5, max_iters=iters, init=A.kmeans_init(X))


@functools.lru_cache(maxsize=None)
def tsne_P():
    return T.affinities(A.tsne_points(), 5.0)


@functools.lru_cache(maxsize=None)
def ref_tsne(d2, iters):
    return T.run(tsne_P(), A.tsne_start(128, d2), iters=iters, exaggeration_iters=2, exact=True)


@functools.lru_cache(maxsize=None)
def ref_index(name, D, metric, nprobe, k=10):
    X = A.matrix(name, D)[0]
    lab, C = A.given_index(D)
    q = np.arange(N, dtype=np.uint32)
    return index_ref.index_ref(X, lab, C, k, metric, nprobe, qids=q, rowptr=A.graph()[0], colids=A.graph()[1], exclude_self=True,
                               S=ref_scores(name, D, metric))


def logreg_case(name, D, feature):
    """-> (X, a, b or None, features float32 [m, D], W)"""
    X, classes = A.matrix(name, D)
    a, b = A.logreg_pairs(A.matrix("nonfinite", D)[1])
    if feature is None:
        b = None
    with np.errstate(all="ignore"):
        Fm = LR.features(X, a, b, LR.FEATURES[feature] if feature else LR.HADAMARD)
    return X, a, b, Fm, A.logreg_weights(D)


def subnormal(s):
    s = np.asarray(s)
    with np.errstate(invalid="ignore"):
        return (s != 0) & (np.abs(s) < E.FLT_MIN)


# ---- host: the inputs say something --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D", MD)
def test_nearest_results_say_something(name, D):
    """At least half the returned scores are finite in every (matrix, D, metric); `finite` at D = 16 has subnormal dot and L2 scores and
    queries whose cosine scores hold both zeros; `nonfinite` returns NaN and infinite scores; `tiny` is all subnormal products."""
    for metric in METRICS:
        for form in ("all", "few"):
            ids, sc = ref_rows(name, D, metric, 0, form)
            assert np.isfinite(sc).mean() >= 0.5, (metric, form, np.isfinite(sc).mean())
    if name == "finite":
        assert subnormal(ref_rows(name, D, "dot", 0, "all")[1]).any() and subnormal(ref_rows(name, D, "l2", 0, "all")[1]).any()
        ids, sc = ref_rows(name, D, "cos", 0, "all")
        neg, pos = (sc == 0) & np.signbit(sc), (sc == 0) & ~np.signbit(sc)
        both = neg.any(axis=1) & pos.any(axis=1)
        assert both.sum() >= 2  # -0 and +0 in one result: the tie rule has to fold them
        for q in A.matrix(name, D)[1]["1e-40"]:  # a query with r = 0: EVERY score is a zero of the dot product's sign, ids ascending
            assert (sc[q] == 0).all() and 30 <= np.signbit(sc[q]).sum() <= 98 and np.array_equal(ids[q], np.arange(128))
        assert A.matrix(name, D)[1]["1e-40"][0] in queries_of(name, D, "few")
    if name == "nonfinite":
        for metric in METRICS:
            sc = ref_rows(name, D, metric, 0, "all")[1]
            assert np.isnan(sc).any() and (np.isinf(sc).any() or metric == "cos"), metric
        assert np.isposinf(ref_rows(name, D, "dot", 0, "all")[1]).any()
    if name == "tiny":
        assert subnormal(ref_scores(name, D, "dot")).mean() >= 0.15 and np.isfinite(ref_scores(name, D, "cos")).all()
        assert (np.abs(ref_scores(name, D, "cos")) > 0.01).mean() >= 0.5  # cosines of size 0.1 from subnormal dot products
    if name == "huge":
        assert np.abs(ref_scores(name, D, "l2")).max() >= 1e37


@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "nonfinite") for D in DIMS])
def test_scores_obey_the_rules_class_by_class(name, D):
    """Every (planted row | vector query, planted row | a few ordinary rows) pair whose score the hand-stated rules decide: the
    restatement has that score, in both orders.  Then the rules one by one, on the classes that show them."""
    X, classes = A.matrix(name, D)
    planted = A.planted_rows(classes)
    others = planted + [0, 1, 2, 150, 299]
    Q = A.vector_queries(D)
    decided = {m: 0 for m in METRICS}
    for metric in METRICS:
        Sr, Sv = ref_scores(name, D, metric), ref_scores(name, D, metric, True)
        for p in planted:
            for o in others:
                for q, c in ((p, o), (o, p)):
                    try:
                        want = A.expected_score(metric, X[q], X[c])
                    except NotSpecial:
                        continue
                    decided[metric] += 1
                    assert np.array_equal(Sr[q, c], want, equal_nan=True), (metric, E.class_of(classes, q), q, E.class_of(classes, c), c, float(Sr[q, c]), float(want))
        for v in range(len(Q)):
            for c in others:
                try:
                    want = A.expected_score(metric, Q[v], X[c])
                except NotSpecial:
                    continue
                decided[metric] += 1
                assert np.array_equal(Sv[v, c], want, equal_nan=True), (metric, A.QUERY_NAMES[v], E.class_of(classes, c), c, float(Sv[v, c]), float(want))
    assert min(decided.values()) >= 100, decided
    dot, l2, cos = (ref_scores(name, D, m) for m in METRICS)
    clean = np.isfinite(X).all(axis=1)
    # dot from +0 never yields -0 where every product is an exact zero (the -0 row, the zero and -0 queries)
    z = classes["negzero"][0]
    assert (dot[clean, z] == 0).all() and not np.signbit(dot[clean, z]).any() and not np.signbit(dot[z, clean]).any()
    assert not np.signbit(ref_scores(name, D, "dot", True)[:2][:, clean]).any()
    # L2 of equal rows is a zero (the call reports +0)
    a, b = classes["equal"]
    assert l2[a, b] == 0 and l2[b, a] == 0 and (np.diagonal(l2)[clean] == 0).all()
    # a row whose squares all underflow: cosine r = 0, every cosine score with a finite row is a zero of the dot product's sign
    for r in classes["1e-40"]:
        assert A.squared_norm_class(X[r]) == "zero" and (cos[r, clean] == 0).all() and (cos[clean, r] == 0).all()
        assert np.array_equal(np.signbit(cos[clean, r]), np.signbit(dot[clean, r])) and np.signbit(cos[clean, r]).any() and not np.signbit(cos[clean, r]).all()
    # a row whose squared norm overflows has r = 0: 0 where the dot product is finite, NaN where it is infinite
    big = [r for r in classes["3e18"] + classes.get("1e19", []) if A.squared_norm_class(X[r]) == "inf"]
    assert big or D == 16
    for r in big:
        fin, inf = clean & np.isfinite(dot[:, r]), np.isinf(dot[:, r])
        assert fin.sum() >= 200 and (cos[fin, r] == 0).all() and np.isnan(cos[inf, r]).all()
    if name == "nonfinite":
        assert D == 16 or any(np.isinf(dot[:, r]).any() for r in big)
        # any score with the NaN row is a NaN
        nan = classes["nan_row"][0]
        assert all(np.isnan(s[nan]).all() and np.isnan(s[:, nan]).all() for s in (dot, l2, cos))
    # L2 to a row of 3e18 is -inf where the chain overflows, and ranks below every number and above a NaN
    if big:
        r = big[0]
        assert np.isneginf(l2[0, r])
        ids, sc = R.top_k(l2[:1], N)
        at = int(np.flatnonzero(ids[0] == r)[0])
        assert not np.isnan(sc[0, :at]).any() and (sc[0, :at] >= sc[0, at]).all() and (np.isnan(sc[0, at + 1:]) | np.isneginf(sc[0, at + 1:])).all()
        assert name == "finite" or np.isnan(sc[0, -1])


@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "nonfinite") for D in (16, 128)])
def test_ranking_obeys_the_rules(name, D):
    """The restatement's order, checked place by place against the ranking stated by hand: a number before a NaN, -0 = +0, equal scores
    and NaNs by ascending id, every candidate once, padding behind."""
    classes = A.matrix("nonfinite", D)[1]
    rowptr, colids = A.graph()
    for metric in METRICS:
        Sr = ref_scores(name, D, metric)
        q = A.few_queries(classes)
        for flags in (0, 3):
            mask = R.exclusion_mask(q, N, rowptr, colids, bool(flags & 1), bool(flags & 2)) if flags else np.zeros((len(q), N), dtype=bool)
            ids, sc = R.top_k(Sr[q], N, mask)
            for i in range(len(q)):
                assert A.check_order(ids[i], sc[i], np.flatnonzero(~mask[i])) is None, (metric, flags, int(q[i]), A.check_order(ids[i], sc[i], np.flatnonzero(~mask[i])))
        ids, sc = R.top_k(ref_scores(name, D, metric, True), N)
        for i in range(len(ids)):
            assert A.check_order(ids[i], sc[i], range(N)) is None, (metric, A.QUERY_NAMES[i])
    if name == "nonfinite":  # NaNs among themselves by ascending id: the NaN row's own result
        nan = classes["nan_row"][0]
        ids, sc = R.top_k(ref_scores(name, D, "dot")[nan:nan + 1], N)
        assert np.isnan(sc).all() and np.array_equal(ids[0], np.arange(N))
    # the check itself notices a -0 ranked below a +0 of a higher id, and a NaN in front
    assert A.check_order([1, 0], [F32(0.0), F32(-0.0)], [0, 1]) is not None and A.check_order([0, 1], [F32(-0.0), F32(0.0)], [0, 1]) is None
    assert A.check_order([0, 1], [F32(np.nan), F32(1.0)], [0, 1]) is not None and A.check_order([1, 0], [F32(-np.inf), F32(np.nan)], [0, 1]) is None


@pytest.mark.parametrize("D", (16, 128))
def test_index_probe_order_has_a_zero_tie(D):
    """Lists 1 and 2 score +0 and -0 (or -0 and +0) under the cosine for every query: one score, so list 1 is probed first.  With
    nprobe = 2 the probes of many queries hold list 1 where list 2 has the +0."""
    X = A.matrix("finite", D)[0]
    lab, C = A.given_index(D)
    SC = R.scores(X, C, "cos")
    assert A.squared_norm_class(C[1]) == "zero" == A.squared_norm_class(C[2])
    clean = np.flatnonzero(np.isfinite(X).all(axis=1) & (R.chain_sq(X) > 0) & np.isfinite(R.chain_sq(X)))
    assert (SC[clean][:, 1:3] == 0).all() and (np.signbit(SC[clean, 1]) != np.signbit(SC[clean, 2])).all()
    probes = ref_index("finite", D, "cos", 2)[2]
    told = [q for q in clean if np.signbit(SC[q, 1]) and 1 in probes[q] and 2 not in probes[q]]
    assert len(told) >= 20, len(told)
    both = [q for q in clean if list(probes[q]) == [1, 2]]
    assert len(both) >= 5, len(both)


@pytest.mark.parametrize("D", (16, 128))
def test_kmeans_inputs_say_something(D):
    for name in ("finite", "tiny", "huge"):
        res = ref_kmeans(name, D)
        assert np.isfinite(res.centroids).all() and (res.counts > 0).all() and res.iterations >= 2, (name, res.iterations, res.counts)
        assert np.isfinite(res.inertia) or name == "finite"
    dist = K.assign(A.matrix("tiny", D)[0], ref_kmeans("tiny", D).centroids)[1]
    assert (dist > 0).all() and dist.max() < 1e-36  # sums of subnormal squares: every distance is 0 where they are flushed
    # rows with an inf, or of 1e19: every distance is +inf, the label is 0 by the tie rule and the inertia is +inf
    X, classes = A.matrix("inf_only", D)
    assert set(classes) == {c for c, _ in E.FINITE_CLASSES} | {"1e19", "inf_one", "ninf_last"} and not np.isnan(X).any()
    first = ref_kmeans("inf_only", D, 0)
    rows = [classes[c][0] for c in ("inf_one", "ninf_last", "1e19")]
    lab, dist = K.assign(X, A.kmeans_init(X))
    assert np.isposinf(dist[rows]).all() and (first.labels[rows] == 0).all() and first.inertia == np.inf and len(set(first.labels.tolist())) == 5
    later = ref_kmeans("inf_only", D)
    assert later.inertia == np.inf and later.iterations >= 1


@pytest.mark.parametrize("which,name,D", SEP_CASES)
def test_silhouette_obeys_the_rules(which, name, D):
    """b(i) and its cluster by `replaced only where m < b`, s(i) from a(i) and b(i) by rule, on every sample of every case; and the
    conditions: (c) and the finite cases keep at least half the samples finite, (b) and (c) on `nonfinite` hold NaN samples, in (b) a
    sample has a NaN b(i) beside a number a(i)."""
    X, lab, classes = silhouette_case(which, name, D)
    sil = ref_separation(which, name, D)[0]
    a, means = silhouette_parts(which, name, D)
    counts = np.bincount(lab)
    nan_b_number_a = 0
    for i in range(N):
        cand = [(c, means[i, c]) for c in range(len(counts)) if c != lab[i]]
        b, other = A.expected_b(cand)
        assert other == sil.other[i] and A.same_bits(np.array([A.expected_s(a[i], b, counts[lab[i]])]), sil.s[i:i + 1]), (i, a[i], b, sil.s[i])
        nan_b_number_a += bool(np.isnan(b) and np.isfinite(a[i]))
    finite = np.isfinite(sil.s).mean()
    if which == "b" and name == "nonfinite":
        # cluster 0 holds the NaN row, and it is every other sample's FIRST candidate: b(i) is a NaN for all of them while a(i) is a
        # number -- with fmin in place of `m < b` every one of these samples would be finite
        assert nan_b_number_a >= N - 32 - 4 and np.isnan(sil.s).all()
        assert np.isfinite(np.where(np.isnan(means), np.inf, means).min(axis=1)).mean() >= 0.5  # what an fmin would have returned
    else:
        assert finite >= 0.5, finite
    if which == "c" and name == "nonfinite":
        assert np.isnan(sil.s).any() and nan_b_number_a == 0 and finite >= 0.85
        assert np.isnan(means[:, 4]).all()  # the NaN mean is there, as the LAST candidate: it never enters
    if which == "a" and name == "finite" and D == 128:
        inf_a = np.isposinf(a)
        assert inf_a.any() and np.isnan(sil.s[inf_a]).all()  # a sample whose own cluster sum is inf has s = NaN
    if which == "d":
        e0, e1 = A.coincident_case(D)[2]["equal"]
        assert a[e0] == 0.0 and means[e0, 2] == 0.0 and sil.s[e0] == 0.0 and sil.s[e1] == 0.0 and sil.other[e0] == 2  # a = 0 = b: s = 0
        assert means[e0, 1] > 0.0


@pytest.mark.parametrize("D", (16, 128))
def test_davies_bouldin_obeys_the_rules(D):
    """Case (d): R_cd is +inf for coincident centroids with a scatter, 0 where both scatters vanish; the score is the mean of the
    clusters' largest R, +inf here."""
    X, lab, rows = A.coincident_case(D)
    db = ref_separation("d", "finite", D)[1]
    assert np.array_equal(db.centroids[0], db.centroids[1]) and np.array_equal(db.centroids[0], db.centroids[2]) and np.array_equal(db.centroids[0], X[1])
    assert db.scatter[0] == 0.0 and db.scatter[2] == 0.0 and db.scatter[1] > 0.0 and list(db.counts[:3]) == [2, 2, 1]
    M = S.distances(db.centroids, db.centroids).astype(F64)
    assert A.expected_r(db.scatter[0], db.scatter[2], M[0, 2]) == 0.0 and A.expected_r(db.scatter[0], db.scatter[1], M[0, 1]) == np.inf
    total = 0.0
    for c in range(5):
        total += max(A.expected_r(db.scatter[c], db.scatter[d], M[c, d]) for d in range(5) if d != c)
    assert db.score == total / 5.0 == np.inf
    # the other cases: finite scores on the finite matrices
    for name in ("finite", "tiny", "huge"):
        other = ref_separation("a", name, D)[1]
        assert np.isfinite(other.centroids).all() and (np.isfinite(other.score) or (name == "finite" and D == 128)), (name, other.score)


@pytest.mark.parametrize("D", (16, 100))
def test_pca_inputs_say_something(D):
    """PCA converges with a finite variance on the three finite matrices (fp64 chains over fp32 inputs of 3e18 and 1e-20)."""
    for name in ("finite", "tiny", "huge"):
        p = ref_pca(name, D)
        assert p.converged and p.sweeps < L.MAX_SWEEPS and np.isfinite(p.variance).all() and (p.variance > 0).all() and np.isfinite(p.y).all(), (name, p.sweeps)
        assert np.isfinite(p.total_variance) and p.variance[0] >= p.variance[1]
    assert ref_pca("finite", D).variance[0] > 1e34 and ref_pca("tiny", D).variance[0] < 1e-37


def test_pca_of_a_matrix_with_a_nan_column():
    """With a NaN in one column the mean is a NaN in that column alone, the eigenproblem is poisoned, and the Jacobi method runs its 64
    sweeps without converging."""
    X, classes = A.matrix("nan_column", 16)
    m = L.mean(X)
    assert np.flatnonzero(np.isnan(m)).tolist() == [1] and m[15] == -np.inf and np.isfinite(np.delete(m, [1, 15])).all()
    with np.errstate(all="ignore"):
        lam, V, sweeps, converged = L.jacobi(L.scatter(X, m))
    assert sweeps == L.MAX_SWEEPS and not converged


def test_tsne_start_obeys_the_rules():
    """A coincident pair and a pair whose squares underflow give w = 1; the pair with a = inf gives w = 0 and r = 0, not a NaN; every
    row stays finite over 3 iterations."""
    for d2 in (2, 3):
        y0 = A.tsne_start(128, d2)
        yf = y0.astype(F32)
        assert np.signbit(yf[5, 0]) and yf[5, 0] == 0 and not np.signbit(yf[5, 1])
        with np.errstate(all="ignore"):
            t, w = T._pair(yf[:, None, :], yf[None, :, :])
            r = (w * w)[:, :, None] * t
        special = 0
        for i in range(128):
            for j in range(128):
                try:
                    we, re = A.expected_tsne_pair(yf[i], yf[j])
                except NotSpecial:
                    continue
                special += i != j
                assert w[i, j] == we and E.same_values(r[i, j], re), (i, j)
        c0, c1 = A.TSNE_SPECIAL["coincident"]
        u0, u1 = A.TSNE_SPECIAL["underflow"]
        f0, f1 = A.TSNE_SPECIAL["far"]
        assert special == 16 and w[c0, c1] == 1 and not t[c0, c1].any() and w[u0, u1] == 1 and t[u0, u1].any()
        assert w[f0, f1] == 0 and np.isfinite(t[f0, f1]).all() and not r[f0, f1].any() and not np.isnan(r).any()
        assert subnormal(w[f0, 8:]).all()  # 1 / (1 + 1e38)
        rowptr, colids, _ = tsne_P()
        for i, j in ((c0, c1), (u0, u1), (f0, f1)):  # nonzeros of P: the attraction and the KL sum meet w = 1 and w = 0 too
            assert j in colids[rowptr[i]:rowptr[i + 1]] and i in colids[rowptr[j]:rowptr[j + 1]]
        for iters in (1, 3):
            res = ref_tsne(d2, iters)
            assert np.isfinite(res.y).all() and np.isfinite(res.z) and np.isfinite(res.kl), (d2, iters)
        assert np.abs(ref_tsne(d2, 3).y[8:]).max() > 1e-3  # the ordinary points have moved


@pytest.mark.parametrize("D", (16, 128))
def test_logreg_inputs_say_something(D):
    """The restated features keep a subnormal product, inf x 0 is a NaN in the chain, and most decision values stay finite."""
    for feature in FEATURES:
        for name in ("finite", "tiny", "nonfinite"):
            X, a, b, Fm, W = logreg_case(name, D, feature)
            with np.errstate(all="ignore"):
                z = LR.logits(Fm, W)
            assert np.isfinite(z).mean() >= 0.5, (feature, name)
            if name == "tiny" and feature in ("hadamard", "l2"):
                assert subnormal(Fm).mean() >= 0.5 and W[2, -1] == 0.0 and (z[:, 2] != 0).mean() >= 0.8 and np.abs(z[:, 2]).max() < 1e-35  # (a zero bias: they are the whole value)
            if name == "nonfinite":
                assert np.isnan(z).any() and (np.isinf(z).any() or feature == "hadamard")
    # inf x 0: the class whose first weights are zero meets the row with an inf in dimension 1
    X, classes = A.matrix("nonfinite", D)
    r = classes["inf_one"][0]
    W = A.logreg_weights(D)
    with np.errstate(all="ignore"):
        z = LR.logits(X[r:r + 1], W)
    assert W[1, 1] == 0.0 and np.isnan(z[0, 1]) and np.isinf(z[0, 0])


def test_restated_fma_takes_infinite_operands():
    """fma24 with an infinite feature or accumulator has the fma's value (it was inf - inf = NaN from the two-sum's error term)."""
    inf = np.inf
    got = LR.fma24(np.array([inf, inf, 2.0, -inf, 1.5]), np.array([2.0, 0.0, 3.0, 1.0, 0.1]), np.array([1.0, 1.0, inf, inf, 0.2]))
    assert got[0] == inf and np.isnan(got[1]) and got[2] == inf and np.isnan(got[3]) and got[4] == LR.fma24(np.array([1.5]), np.array([0.1]), np.array([0.2]))[0]


def test_same_bits_tells_zeros_and_widths_apart():
    assert A.same_bits(np.array([0.0, np.nan, np.inf]), np.array([0.0, -np.nan, np.inf])) and not A.same_bits(np.array([0.0]), np.array([-0.0]))
    assert not A.same_bits(np.array([1.0], dtype=F32), np.array([1.0])) and not A.same_bits(np.array([np.nan]), np.array([1.0]))
    assert A.same_bits(np.array([-0.0], dtype=F32), np.array([-0.0], dtype=F32)) and not A.same_bits(np.array([5e-324]), np.array([0.0]))
    assert A.no_negative_zero(np.array([0.0, -1.0, np.nan], dtype=F32)) and not A.no_negative_zero(np.array([1.0, -0.0], dtype=F32))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def engine_for(X):
    eng = F.Engine(*A.graph(len(X)), X.shape[1])
    eng.set_embeddings(np.array(X))
    return eng


def nearest_ok(got, want, what):
    assert got[1].dtype == F32 and R.same(got, want), what
    assert A.no_negative_zero(got[1]), ("a zero with its sign bit set", what)


@gpu
@pytest.mark.parametrize("name,D", MD)
def test_nearest_rows_equal_the_restatement(name, D):
    """Every row as a query (the 128-query form where D <= 128) and 20 rows (the 32-query form), flags 0 and 3, k = 1, 10, 128, one and
    three candidate splits, the three metrics."""
    X = A.matrix(name, D)[0]
    eng = engine_for(X)
    try:
        for splits in (1, 3):
            eng.set_param("nearest_splits", splits)
            for metric in METRICS:
                for flags in (0, 3):
                    for form in ("all", "few"):
                        q = queries_of(name, D, form)
                        ids, sc = ref_rows(name, D, metric, flags, form)
                        for k in KS:
                            got = eng.nearest(ids=q, k=k, metric=metric, exclude_self=bool(flags & 1), exclude_neighbours=bool(flags & 2))
                            nearest_ok(got, (ids[:, :k], sc[:, :k]), (splits, metric, flags, form, k))
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name,D", MD)
def test_nearest_vectors_equal_the_restatement(name, D):
    """Queries that are no rows: a zero vector, a -0 vector, a 1e-40 vector, FLT_MAX in one component, a NaN in one component."""
    X = A.matrix(name, D)[0]
    eng = engine_for(X)
    try:
        for splits in (1, 3):
            eng.set_param("nearest_splits", splits)
            for metric in METRICS:
                ids, sc = ref_vectors(name, D, metric)
                for k in KS:
                    nearest_ok(eng.nearest(vectors=A.vector_queries(D), k=k, metric=metric), (ids[:, :k], sc[:, :k]), (splits, metric, k))
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "nonfinite") for D in (16, 128)])
def test_index_search_equals_the_restatement(name, D):
    """A caller-given index (labels arange % 5, two centroids whose cosine scores are the two zeros): nprobe = lists is the exhaustive
    result, and nprobe = 2 under the cosine has the +-0 tie in its probe order."""
    X = A.matrix(name, D)[0]
    lab, C = A.given_index(D)
    q = np.arange(N, dtype=np.uint32)
    eng = engine_for(X)
    try:
        eng.build_index(labels=lab, centroids=C)
        for metric, nprobe in [(m, 5) for m in METRICS] + [("cos", 2), ("dot", 2)]:
            ids, sc, probes, cand = ref_index(name, D, metric, nprobe)
            got = eng.index_search(ids=q, k=10, metric=metric, nprobe=nprobe, exclude_self=True, details=True)
            nearest_ok(got[:2], (ids, sc), (metric, nprobe))
            assert np.array_equal(got[2], probes) and got[3]["candidates"] == cand, (metric, nprobe)
            if nprobe == 5:
                nearest_ok(got[:2], tuple(a[:, :10] for a in ref_rows(name, D, metric, 1, "all")), (metric, "exhaustive"))
        Q = A.vector_queries(D)
        for metric in METRICS:
            want = index_ref.index_ref(X, lab, C, 10, metric, 2, vectors=Q)
            got = eng.index_search(vectors=Q, k=10, metric=metric, nprobe=2, details=True)
            nearest_ok(got[:2], want[:2], (metric, "vectors"))
            assert np.array_equal(got[2], want[2]), metric
    finally:
        eng.close()


def kmeans_ok(got, want, what):
    assert np.array_equal(got.labels, want.labels) and np.array_equal(got.counts, want.counts), what
    assert A.same_bits(got.centroids, want.centroids), (what, E.difference(got.centroids, want.centroids))
    assert A.same_bits(np.array([got.inertia]), np.array([want.inertia])), (what, got.inertia, want.inertia)
    assert got.iterations == want.iterations and bool(got.converged) == bool(want.converged), what


@gpu
@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "tiny", "huge", "inf_only") for D in (16, 128)])
def test_kmeans_equals_the_restatement(name, D):
    X = A.matrix(name, D)[0]
    eng = engine_for(X)
    try:
        for iters in (6, 0) if name == "inf_only" else (6,):
            want = ref_kmeans(name, D, iters)
            kmeans_ok(eng.kmeans(5, max_iters=iters, init=A.kmeans_init(X)), want, (name, D, iters))
            if name == "inf_only":
                assert want.inertia == np.inf
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("which,name,D", SEP_CASES)
def test_separation_equals_the_restatement(which, name, D):
    X, lab, _ = silhouette_case(which, name, D)
    sil, db = ref_separation(which, name, D)
    eng = engine_for(X)
    try:
        score, s, other = eng.silhouette(lab, samples=True)
        dscore, centroids, scatter, counts = eng.davies_bouldin(lab, details=True)
    finally:
        eng.close()
    bad = np.flatnonzero(~((np.isnan(s) & np.isnan(sil.s)) | (s.view(np.uint64) == sil.s.view(np.uint64))))
    assert A.same_bits(s, sil.s), ("s(i)", len(bad), int(bad[0]), s[bad[0]], sil.s[bad[0]])
    assert np.array_equal(other, sil.other) and A.same_bits(np.array([score]), np.array([sil.score])), (score, sil.score)
    assert A.same_bits(centroids, db.centroids) and A.same_bits(scatter, db.scatter) and np.array_equal(counts, db.counts)
    assert A.same_bits(np.array([dscore]), np.array([db.score])), (dscore, db.score)


@gpu
@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "tiny", "huge") for D in (16, 100)])
def test_pca_equals_the_restatement(name, D):
    want = ref_pca(name, D)
    eng = engine_for(A.matrix(name, D)[0])
    try:
        got = eng.pca(2, details=True)
    finally:
        eng.close()
    assert A.same_bits(got.mean, want.mean) and A.same_bits(got.components, want.components) and A.same_bits(got.variance, want.variance)
    assert A.same_bits(np.array([got.info.total_variance]), np.array([want.total_variance]))
    assert got.info.sweeps == want.sweeps and got.info.converged == want.converged
    assert A.same_bits(got.y, want.y), E.difference(got.y, want.y)


@gpu
def test_pca_of_a_nan_column_returns_its_mean_and_does_not_converge():
    """What is asked of PCA on a non-finite matrix: F2V_OK, the mean a NaN in the planted column alone and bit-equal elsewhere, converged
    = 0 after 64 sweeps.  Everything else of the result is NaN and is not compared."""
    X = A.matrix("nan_column", 16)[0]
    eng = engine_for(X)
    try:
        got = eng.pca(2, details=True)
    finally:
        eng.close()
    assert A.same_bits(got.mean, L.mean(X)) and np.flatnonzero(np.isnan(got.mean)).tolist() == [1]
    assert got.info.sweeps == L.MAX_SWEEPS and not got.info.converged


@gpu
@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "nonfinite") for D in (16, 128)])
def test_trustworthiness_equals_the_restatement(name, D):
    X = A.matrix(name, D)[0]
    Y = np.ascontiguousarray(X[:, :2])
    want = L.trust(X, Y, 10)
    eng = engine_for(X)
    try:
        got = eng.trustworthiness(Y, k=10, samples=True)
    finally:
        eng.close()
    assert np.array_equal(got.samples_x, want.samples_x) and np.array_equal(got.samples_y, want.samples_y)
    assert (int(got.penalty_x), int(got.penalty_y), int(got.hits)) == (want.penalty_x, want.penalty_y, want.hits)
    assert want.penalty_x > 0 and want.penalty_y > 0


@gpu
@pytest.mark.parametrize("d2,iters", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_tsne_iteration_equals_the_restatement(d2, iters):
    """The pair kernels at a = 0 (coincident points, squares that underflow), a = inf (w = 0 while t is finite), a subnormal w, a -0
    coordinate -- P is the restatement's, passed in, so nothing depends on the device's exp."""
    want = ref_tsne(d2, iters)
    eng = engine_for(A.tsne_points())
    try:
        y, info = eng.tsne(d2, iters=iters, P=tsne_P(), init=A.tsne_start(128, d2), exaggeration_iters=2, details=True)
    finally:
        eng.close()
    assert A.same_bits(y, want.y), E.difference(y, want.y)
    assert A.same_bits(np.array([info["kl"], info["z"]]), np.array([want.kl, want.z])), (info["kl"], want.kl, info["z"], want.z)


@gpu
@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "tiny", "nonfinite") for D in (16, 128)])
def test_logreg_decision_equals_the_restatement(name, D):
    """The four pair features and the rows form: fp32 features (a subnormal product kept, inf - inf, inf x 0), fp64 fma chains."""
    eng = engine_for(A.matrix(name, D)[0])
    try:
        for feature in FEATURES:
            X, a, b, Fm, W = logreg_case(name, D, feature)
            with np.errstate(all="ignore"):
                want = LR.logits(Fm, W)
            got = eng.logreg_decision(W, ids=a) if b is None else eng.logreg_decision(F.LogregModel(W, feature, *[None] * 6), pairs=(a, b))
            bad = np.argwhere(~((np.isnan(got) & np.isnan(want)) | (got == want)))
            assert A.same_bits(got, want), (feature, len(bad), bad[:1].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name,D", [(name, D) for name in ("finite", "tiny") for D in (16, 128)])
def test_logreg_eval_is_close_to_the_restatement(name, D):
    eng = engine_for(A.matrix(name, D)[0])
    try:
        for feature in FEATURES:
            X, a, b, Fm, W = logreg_case(name, D, feature)
            y = np.random.default_rng(17).integers(0, 2, (len(a), len(W))).astype(np.uint8)
            with np.errstate(over="ignore"):
                want = LR.eval_sums(Fm, y, W, lam=0.7)
            loss, grad = eng.logreg_eval(W, y, ids=a if b is None else None, pairs=None if b is None else (a, b), feature=feature or "hadamard", lam=0.7)
            assert np.all(np.isfinite(loss)) and np.all(np.isfinite(grad)), feature
            assert close_enough(loss, want.loss, want.loss_abs) and close_enough(grad, want.grad, want.grad_abs), feature
    finally:
        eng.close()
