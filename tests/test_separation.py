"""GPU silhouette and Davies-Bouldin scores of a labelling (include/f2v.h: f2v_silhouette, f2v_davies_bouldin; Engine.silhouette /
Engine.davies_bouldin; the CLI's -separation).

Host tests (no GPU): argument checks, the exported constants, the CLI's refusals before the graph is read, the compiled gfx950 code
of every kernel of f2v_separation.hip.h (no scratch, nothing spilled, both builds), and the numpy restatement of the definition
(tests/separation_ref.py) against scikit-learn.  -m gpu: score, every s(i), every other(i), centroids, scatter and counts bit for bit
against the restatement; empty, singleton, unlabelled and coincident cases; sample subsets; independence of calls, handles and
tunables; non-interference with training; every error case; a trained cora embedding; the CLI's line.

The restatement emulates every fp32 fma in fp64 arithmetic (about 2e7 pair-dimensions a second), so where n^2 D is large the
bit-for-bit comparison of the silhouette takes a seeded subset of the samples -- each still scored against ALL labelled vertices, as
the definition has it -- and a full call on the GPU must return the same s(i) for those vertices."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import separation_ref as S
from test_gather_isa import FLAGS, HIPCC, function
from test_kmeans import blobs, engine_for, noise, spills

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu
NONE = _lib.LABEL_NONE

# The restatement against scikit-learn (float64 copies of the inputs) on the five inputs of SKLEARN_INPUTS, as measured with the
# restatement as committed: max |s(i) - silhouette_samples| 8.27e-9, 6.19e-9, 9.88e-9, 2.06e-8, 1.89e-8; relative Davies-Bouldin
# difference 1.12e-8, 7.61e-8, 2.9e-8, 6.13e-8, 1.46e-8.  The differences are those of fp32 distances against fp64 ones and scale with
# the values: 16 times the largest seen is allowed.
SIL_TOL = 16 * 2.06e-8
DB_RTOL = 16 * 7.61e-8


def blob_labels(n, D, k, seed):
    """test_kmeans.blobs and the component that generated every row (the generator's own draw order)."""
    rng = np.random.default_rng(seed)
    rng.standard_normal((k, D))
    return blobs(n, D, k, seed), rng.integers(0, k, n)


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_null_and_bad_arguments():
    L = _lib.lib()
    labels = np.zeros(8, dtype=np.uint32)
    score = C.c_double()
    lp = labels.ctypes.data_as(_lib.u32p)
    assert L.f2v_silhouette(None, lp, 2, None, 0, None, None, C.byref(score), None) == _lib.F2V_EINVAL
    assert b"null" in L.f2v_last_error()
    assert L.f2v_davies_bouldin(None, lp, 2, C.byref(score), None, None, None, None) == _lib.F2V_EINVAL
    assert b"null" in L.f2v_last_error()
    want = (0xFFFFFFFF, 1024, 64, 64)
    assert (F.LABEL_NONE, F.SEPARATION_MAX_CLUSTERS, F.SEPARATION_PIECE, F.SEPARATION_SPAN) == want
    assert (_lib.LABEL_NONE, _lib.SEPARATION_MAX_CLUSTERS, _lib.SEPARATION_PIECE, _lib.SEPARATION_SPAN) == want
    assert "f2v_silhouette" in _lib.SIGNATURES and "f2v_davies_bouldin" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "f2v.h")).read()
    for line in ("#define F2V_LABEL_NONE 0xFFFFFFFFu", "#define F2V_SEPARATION_MAX_CLUSTERS 1024", "#define F2V_SEPARATION_PIECE 64",
                 "#define F2V_SEPARATION_SPAN 64"):
        assert line in header, line


@pytest.mark.parametrize("args,word", [(["-separation", "kmeans"], "-separation"), (["-separation-sample", "-1"], "-separation-sample"),
                                       (["-separation", "x", "-gpus", "2"], "-separation")])
def test_cli_rejects_bad_separation_flags_before_reading_the_graph(tmp_path, args, word):
    for mtx in (os.path.join(tmp_path, "missing.mtx"), golden_graph_path("karate.mtx")):
        r = subprocess.run([CLI, "-input", mtx, "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1, r.stdout + r.stderr
        assert word in r.stdout and "Reading input" not in r.stdout, r.stdout
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


KERNELS = ["separation_pair_kernelILi64EE", "separation_pair_kernelILi128EE", "separation_finish_kernel", "separation_piece_kernel",
           "separation_scatter_kernel", "separation_cluster_kernel", "separation_ids_kernel"]
TU = """#include "f2v_separation.hip.h"
template __global__ void f2v::separation_pair_kernel<64>(const f2v::SepPairArgs);
template __global__ void f2v::separation_pair_kernel<128>(const f2v::SepPairArgs);
"""


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "separation_isa.hip"), str(tmp_path / "separation_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


SKLEARN_INPUTS = [("blobs", 300, 128, 7, 10), ("blobs", 257, 100, 3, 5), ("blobs", 130, 5, 2, 5), ("noise", 300, 16, 5, 3), ("blobs", 200, 2, 4, 1)]


def sklearn_input(kind, n, D, k, seed):
    if kind == "blobs":
        return blob_labels(n, D, k, seed)
    return noise(n, D, k, seed), np.random.default_rng(seed + 1000).integers(0, k, n)


@pytest.mark.parametrize("kind,n,D,k,seed", SKLEARN_INPUTS, ids=["%s-n%d-D%d-K%d" % s[:4] for s in SKLEARN_INPUTS])
def test_restatement_agrees_with_scikit_learn(kind, n, D, k, seed):
    metrics = pytest.importorskip("sklearn.metrics")
    X, labels = sklearn_input(kind, n, D, k, seed)
    sil, db = S.silhouette(X, labels), S.davies_bouldin(X, labels)
    X64 = X.astype(np.float64)
    ref_s, ref_db = metrics.silhouette_samples(X64, labels), metrics.davies_bouldin_score(X64, labels)
    ds, ddb = float(np.abs(sil.s - ref_s).max()), abs(db.score - ref_db) / ref_db
    print("%s n=%d D=%d K=%d: max |s - sklearn| %.3g, silhouette %.17g, Davies-Bouldin %.17g (relative difference %.3g)" % (
        kind, n, D, k, ds, sil.score, db.score, ddb))
    assert ds <= SIL_TOL and abs(sil.score - metrics.silhouette_score(X64, labels)) <= SIL_TOL
    assert ddb <= DB_RTOL
    assert np.array_equal(db.counts, np.bincount(labels, minlength=k))


def test_restated_sums_take_pieces_then_spans():
    """The restatement's own three-level sum against a plain loop."""
    a = np.random.default_rng(0).standard_normal(64 * 64 + 200)
    pieces = []
    for p in range(0, len(a), 64):
        s = 0.0
        for x in a[p:p + 64]:
            s += x
        pieces.append(s)
    spans = []
    for p in range(0, len(pieces), 64):
        s = 0.0
        for x in pieces[p:p + 64]:
            s += x
        spans.append(s)
    assert len(spans) == 2 and S.ordered_sum(a) == spans[0] + spans[1]


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def same_silhouette(got, want):
    return got[0] == want.score and np.array_equal(got[1], want.s) and np.array_equal(got[2], want.other)


def same_davies_bouldin(got, want):
    return (got[0] == want.score and np.array_equal(got[1].view(np.uint32), want.centroids.view(np.uint32)) and np.array_equal(got[2], want.scatter) and
            np.array_equal(got[3], want.counts))


def report(name, got, want):
    print("%s: score %.17g/%.17g, s differing %d, other differing %d" % (name, got[0], want.score, int((got[1] != want.s).sum()),
                                                                         int((got[2] != want.other).sum())))


SHAPES = [(300, 128, 7), (257, 100, 3), (130, 5, 2), (200, 512, 4)]


@gpu
@pytest.mark.parametrize("n,D,k", SHAPES, ids=["n%d-D%d-K%d" % s for s in SHAPES])
def test_results_equal_the_restatement_bit_for_bit(n, D, k):
    X, labels = blob_labels(n, D, k, 1000 + n)
    eng = engine_for(X)
    try:
        sil, db = eng.silhouette(labels, samples=True), eng.davies_bouldin(labels, details=True)
        assert eng.silhouette(labels) == sil[0] and eng.davies_bouldin(labels) == db[0] and eng.last_separation_seconds > 0
    finally:
        eng.close()
    want = S.silhouette(X, labels)
    report("n=%d D=%d K=%d" % (n, D, k), sil, want)
    assert same_silhouette(sil, want)
    assert same_davies_bouldin(db, S.davies_bouldin(X, labels))


@gpu
def test_many_short_clusters_equal_the_restatement():
    """K = 130 is above one sweep of candidates, its clusters are shorter than a piece.  400 seeded samples in the restatement."""
    n, D, k = 2100, 64, 130
    X, labels = blob_labels(n, D, k, 3100)
    ids = np.random.default_rng(1).permutation(n)[:400]
    eng = engine_for(X)
    try:
        full, sub, db = eng.silhouette(labels, samples=True), eng.silhouette(labels, ids, samples=True), eng.davies_bouldin(labels, details=True)
    finally:
        eng.close()
    want = S.silhouette(X, labels, ids)
    report("n=%d D=%d K=%d" % (n, D, k), sub, want)
    assert np.bincount(labels).max() < 64 and same_silhouette(sub, want)
    assert np.array_equal(full[1][ids], want.s) and np.array_equal(full[2][ids], want.other) and len(full[1]) == n
    assert same_davies_bouldin(db, S.davies_bouldin(X, labels))


@gpu
def test_a_cluster_of_three_spans_equals_the_restatement():
    """One cluster of 8500 members: two full spans of 4096 and a ragged third -- the span order and the workspace that workgroups
    of different spans share.  256 seeded samples in the restatement, every vertex on the GPU."""
    n, D = 9000, 16
    X = noise(n, D, 3, 77)
    labels = np.full(n, 1, dtype=np.int64)
    rng = np.random.default_rng(5)
    rest = rng.permutation(n)[:500]
    labels[rest[:300]], labels[rest[300:]] = 0, 2
    X[labels == 0] += np.float32(0.75)
    ids = np.concatenate([rng.permutation(n)[:226], rest[:15], rest[300:315]])
    eng = engine_for(X)
    try:
        full, sub, db = eng.silhouette(labels, samples=True), eng.silhouette(labels, ids, samples=True), eng.davies_bouldin(labels, details=True)
    finally:
        eng.close()
    want = S.silhouette(X, labels, ids)
    report("n=%d D=%d, clusters of 300 / 8500 / 200" % (n, D), sub, want)
    assert int((labels == 1).sum()) == 8500 and same_silhouette(sub, want)
    assert np.array_equal(full[1][ids], want.s) and np.array_equal(full[2][ids], want.other)
    assert same_davies_bouldin(db, S.davies_bouldin(X, labels))


@gpu
def test_empty_singleton_unlabelled_and_coincident_members():
    n, D = 300, 16
    X, comp = blob_labels(n, D, 3, 12)
    labels = comp.astype(np.int64) + 1           # cluster 0 stays empty
    labels[labels == 3] = 4                      # ... and so does cluster 3
    labels[7] = 5                                # a singleton: s = 0
    labels[[20, 21]] = 6                         # two identical rows, a cluster of their own: a = 0
    X[21] = X[20]
    none = np.random.default_rng(2).permutation(np.arange(30, n))[:40]
    labels[none] = -1
    eng = engine_for(X)
    try:
        sil, db = eng.silhouette(labels, samples=True), eng.davies_bouldin(labels, details=True)
        as_u32 = np.where(labels < 0, NONE, labels).astype(np.uint32)
        assert same_silhouette(eng.silhouette(as_u32, samples=True), S.silhouette(X, labels))  # 0xFFFFFFFF in an unsigned array
    finally:
        eng.close()
    want = S.silhouette(X, labels)
    report("special labelling", sil, want)
    assert same_silhouette(sil, want) and len(sil[1]) == n - 40
    labelled = np.flatnonzero(labels >= 0)
    assert sil[1][labelled == 7][0] == 0.0 and np.all(sil[1][(labelled == 20) | (labelled == 21)] == 1.0)
    assert not np.isin(sil[2], [0, 3]).any()
    want_db = S.davies_bouldin(X, labels)
    assert same_davies_bouldin(db, want_db) and db[3].tolist()[0] == 0 and db[3][5] == 1 and db[3][6] == 2 and int(db[3].sum()) == n - 40
    assert db[2][5] == 0.0 and db[2][6] == 0.0 and not db[1][0].any() and not db[1][3].any()


@gpu
def test_identical_rows_score_zero():
    X = np.tile(np.random.default_rng(3).standard_normal((1, 24)).astype(np.float32), (150, 1))
    labels = np.arange(150) % 4
    eng = engine_for(X)
    try:
        sil, db = eng.silhouette(labels, samples=True), eng.davies_bouldin(labels, details=True)
    finally:
        eng.close()
    assert sil[0] == 0.0 and not sil[1].any() and db[0] == 0.0 and not db[2].any()
    assert same_silhouette(sil, S.silhouette(X, labels)) and same_davies_bouldin(db, S.davies_bouldin(X, labels))


@gpu
def test_sample_subset_in_shuffled_order_with_duplicates():
    n, D, k = 500, 40, 4
    X, labels = blob_labels(n, D, k, 8)
    rng = np.random.default_rng(9)
    ids = rng.permutation(n)[:150]
    ids = np.concatenate([ids, ids[:20], ids[5:6]])[rng.permutation(171)]
    eng = engine_for(X)
    try:
        full, sub = eng.silhouette(labels, samples=True), eng.silhouette(labels, ids, samples=True)
        one = eng.silhouette(labels, ids[:1], samples=True)
    finally:
        eng.close()
    want = S.silhouette(X, labels, ids)
    assert np.array_equal(sub[1], full[1][ids]) and np.array_equal(sub[2], full[2][ids])
    assert same_silhouette(sub, want) and sub[0] != full[0]
    assert one[0] == one[1][0] == full[1][ids[0]]


@gpu
def test_results_do_not_depend_on_calls_handles_or_tunables():
    n, D, k = 700, 64, 5
    X, labels = blob_labels(n, D, k, 33)
    ids = np.random.default_rng(4).permutation(n)[:333]
    eng = engine_for(X)

    def run(e):
        return e.silhouette(labels, samples=True), e.silhouette(labels, ids, samples=True), e.davies_bouldin(labels, details=True)

    def same(a, b):
        return all(x[0] == y[0] and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:])) for x, y in zip(a, b))

    try:
        base = run(eng)
        assert same(run(eng), base)
        other = engine_for(X)
        try:
            assert same(run(other), base), "second handle"
        finally:
            other.close()
        for name, values, default in (("separation_chunk", (64, 100, 8192), 8192), ("separation_block", (64, 128, 0), 0)):
            for v in values:
                eng.set_param(name, v)
                assert eng.get_param(name) == v and same(run(eng), base), (name, v)
            eng.set_param(name, default)
        eng.set_param("separation_chunk", 100)
        eng.set_param("separation_block", 128)
        assert same(run(eng), base)
        eng.set_param("separation_chunk", 8192)
        eng.set_param("separation_block", 0)
        eng.kmeans(9, 3, seed=2)  # shares the workspace: another k, other labels, other centroids
        eng.nearest(ids=np.arange(50), k=5)
        assert same(run(eng), base), "after f2v_kmeans and f2v_nearest_rows"
        for name, bad in (("separation_block", 32), ("separation_block", 256), ("separation_chunk", 0)):
            with pytest.raises(F.F2VError) as e:
                eng.set_param(name, bad)
            assert e.value.code == _lib.F2V_EINVAL and name in str(e.value)
    finally:
        eng.close()


@gpu
def test_scoring_does_not_change_training_and_sees_pending_rows():
    rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))
    n = len(rowptr) - 1
    labels = np.arange(n) % 3

    def run(score):
        eng = F.Engine(rowptr, colids, 16)
        try:
            eng.srand(1)
            eng.init_embeddings(0)
            eng.train(5, 3, 16, 5, 0.02)
            if score:
                eng.silhouette(labels, samples=True)
                eng.davies_bouldin(labels)
            eng.train(5, 3, 16, 5, 0.02)
            return eng.get_embeddings(), eng.rand_index(1 << 30)
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1]
    eng = F.Engine(rowptr, colids, 16)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        ids = eng.draw_samples(n - 1, 5)
        eng.minibatch_step(5, 0, n // 2, ids, 5, 0.02)  # a partial range pending: the scores see what get_embeddings returns
        sil, db = eng.silhouette(labels, samples=True), eng.davies_bouldin(labels, details=True)
        X = eng.get_embeddings()
        assert same_silhouette(sil, S.silhouette(X, labels)) and same_davies_bouldin(db, S.davies_bouldin(X, labels))
    finally:
        eng.close()


@gpu
def test_every_error_case_is_refused_and_training_goes_on():
    rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 16)
    try:
        L, h = eng._L, eng._h
        score = C.c_double()
        u32 = lambda a: a.ctypes.data_as(_lib.u32p)
        good = (np.arange(n) % 3).astype(np.uint32)

        def sil(labels=good, k=3, ids=None, nq=0, out=score):
            return L.f2v_silhouette(h, u32(labels) if labels is not None else None, k, u32(ids) if ids is not None else None, nq, None, None,
                                    C.byref(out) if out is not None else None, None)

        def db(labels=good, k=3, out=score):
            return L.f2v_davies_bouldin(h, u32(labels) if labels is not None else None, k, C.byref(out) if out is not None else None, None, None, None, None)

        assert sil() == db() == _lib.F2V_ESTATE  # before init_embeddings
        eng.srand(1)
        eng.init_embeddings(0)
        bad_label, one_cluster, all_alone = good.copy(), np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)
        bad_label[5] = 3
        one_cluster[3] = NONE
        unlabelled = good.copy()
        unlabelled[4] = NONE
        cases = [("null labels", lambda: sil(labels=None)), ("null score", lambda: sil(out=None)), ("k = 0", lambda: sil(k=0)),
                 ("k = 1025", lambda: sil(k=1025)), ("a label >= k", lambda: sil(labels=bad_label)),
                 ("a sample id >= n", lambda: sil(ids=np.array([1, n], dtype=np.uint32), nq=2)),
                 ("an unlabelled sample", lambda: sil(labels=unlabelled, ids=np.array([4], dtype=np.uint32), nq=1)),
                 ("nq = 0 with sample ids", lambda: sil(ids=np.array([1], dtype=np.uint32), nq=0)),
                 ("one non-empty cluster", lambda: sil(labels=one_cluster)),
                 ("as many clusters as labelled vertices", lambda: sil(labels=all_alone, k=n)),
                 ("db: null labels", lambda: db(labels=None)), ("db: null score", lambda: db(out=None)), ("db: k = 0", lambda: db(k=0)),
                 ("db: k = 1025", lambda: db(k=1025)), ("db: a label >= k", lambda: db(labels=bad_label)), ("db: one non-empty cluster", lambda: db(labels=one_cluster))]
        for name, call in cases:
            L.f2v_set_param(h, b"no_such_param", 0)  # leaves another message behind
            before = L.f2v_last_error()
            assert call() == _lib.F2V_EINVAL, name
            msg = L.f2v_last_error()
            assert msg and msg != before and (b"f2v_silhouette" in msg or b"f2v_davies_bouldin" in msg), (name, msg)
        assert db(labels=all_alone, k=n) == _lib.F2V_OK  # the Davies-Bouldin score needs two clusters, not a spare vertex
        assert sil(labels=unlabelled) == _lib.F2V_OK and sil(ids=np.array([2, 2], dtype=np.uint32), nq=2) == _lib.F2V_OK
        with pytest.raises(F.F2VError) as e:
            eng.silhouette(np.full(n, 2000))
        assert e.value.code == _lib.F2V_EINVAL
        eng.train(5, 2, 16, 5, 0.02)
        X = eng.get_embeddings()
        assert np.isfinite(X).all() and same_silhouette(eng.silhouette(good, samples=True), S.silhouette(X, good))
    finally:
        eng.close()


@gpu
def test_cora_scores_equal_the_restatement_and_scikit_learn():
    """Option 5, 1200 epochs at batch 256 and D = 128 from srand(1) (the run of test_kmeans' quality test), scored with the ground
    truth of tests/golden/cora.nodes.labels.  No quality level is asserted: nobody has measured one.  The silhouette's restatement
    takes 200 seeded samples (2708^2 x 128 pair-dimensions would take it most of a minute), scikit-learn every vertex."""
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    n = len(rowptr) - 1
    labels = np.full(n, -1, dtype=np.int64)
    for line in open(os.path.join(GOLD, "cora.nodes.labels")):
        t = line.split()
        if len(t) >= 2 and labels[int(t[0]) - 1] < 0:
            labels[int(t[0]) - 1] = int(t[1])
    assert (labels >= 0).all() and labels.max() == 6
    ids = np.random.default_rng(6).permutation(n)[:200]
    eng = F.Engine(rowptr, colids, 128)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        eng.train(5, 1200, 256, 5, 0.02)
        X = eng.get_embeddings()
        full = eng.silhouette(labels, samples=True)
        t_sil = eng.last_separation_seconds
        sub, db = eng.silhouette(labels, ids, samples=True), eng.davies_bouldin(labels, details=True)
        print("cora: silhouette %.17g (%.3f ms), of 200 samples %.17g, davies_bouldin %.17g (%.3f ms)" % (
            full[0], t_sil * 1e3, sub[0], db[0], eng.last_separation_seconds * 1e3))
    finally:
        eng.close()
    want = S.silhouette(X, labels, ids)
    assert same_silhouette(sub, want) and np.array_equal(full[1][ids], want.s) and np.array_equal(full[2][ids], want.other)
    assert same_davies_bouldin(db, S.davies_bouldin(X, labels))
    try:
        from sklearn import metrics
    except ImportError:
        return
    X64 = X.astype(np.float64)
    ref_s, ref_db = metrics.silhouette_samples(X64, labels), metrics.davies_bouldin_score(X64, labels)
    print("cora against scikit-learn: max |s - sklearn| %.3g, |score - sklearn| %.3g, Davies-Bouldin relative %.3g" % (
        np.abs(full[1] - ref_s).max(), abs(full[0] - ref_s.mean()), abs(db[0] - ref_db) / ref_db))
    assert np.abs(full[1] - ref_s).max() <= SIL_TOL and abs(full[0] - metrics.silhouette_score(X64, labels)) <= SIL_TOL
    assert abs(db[0] - ref_db) / ref_db <= DB_RTOL


@gpu
def test_cli_prints_the_scores_of_its_own_clusters(tmp_path):
    mtx = golden_graph_path("cora.mtx")
    r = subprocess.run([CLI, "-input", mtx, "-iter", "5", "-dim", "32", "-batch", "256", "-option", "5", "-binout", "1", "-cluster", "7", "-separation", "kmeans",
                        "-output", str(tmp_path) + "/"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^silhouette: (\S+) davies_bouldin: (\S+)$", r.stdout, re.M)
    assert m, r.stdout
    embd = [p for p in os.listdir(tmp_path) if p.endswith(".embd")]
    assert len(embd) == 1
    rowptr, colids = F.read_mtx(mtx)
    n = len(rowptr) - 1
    labels = np.array([int(x.split()[1]) for x in open(str(tmp_path / embd[0]) + ".clu").read().splitlines()], dtype=np.uint32)
    eng = F.Engine(rowptr, colids, 32)
    try:
        eng.set_embeddings(F.read_embd_bin(str(tmp_path / embd[0]) + ".bin", n, 32))
        sil, db = eng.silhouette(labels), eng.davies_bouldin(labels)
        r2 = subprocess.run([CLI, "-input", mtx, "-iter", "5", "-dim", "32", "-batch", "256", "-option", "5", "-notext", "1", "-separation",
                             os.path.join(GOLD, "cora.nodes.labels"), "-separation-sample", "300", "-output", str(tmp_path) + "/"],
                            capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert r2.returncode == 0, r2.stdout + r2.stderr
        m2 = re.search(r"^silhouette: (\S+) davies_bouldin: (\S+)$", r2.stdout, re.M)
        assert m2, r2.stdout
    finally:
        eng.close()
    assert float(m.group(1)) == sil and float(m.group(2)) == db
    assert -1.0 <= float(m2.group(1)) <= 1.0 and float(m2.group(2)) > 0.0 and m2.group(1) != m.group(1)
