"""GPU principal-component layout of the embedding and its trustworthiness (include/f2v.h: f2v_pca, f2v_trustworthiness; Engine.pca /
Engine.trustworthiness; the CLI's -layout).

Host tests (no GPU): argument checks, the exported constants, the CLI's refusals before the graph is read, the compiled gfx950 code of
every kernel of f2v_layout.hip.h (no scratch, nothing spilled, both builds), and the numpy restatement of the definition
(tests/layout_ref.py) against exact rational arithmetic, numpy.linalg and scikit-learn.  -m gpu: mean, components, variances, sweeps
and projection bit for bit against the restatement; every per-sample penalty, the sums and the three scores of f2v_trustworthiness
bit for bit; ties, NaNs and sample lists; identities; independence of calls, handles and tunables; non-interference with training;
every error case; a trained cora embedding; the CLI's line and file.

The restatement emulates every fma in fp64 arithmetic, so where n^2 D is large the comparison of the penalties takes a seeded subset
of the samples -- each still ranked against ALL vertices, as the definition has it -- and a full call on the GPU must return the same
penalties for those vertices."""
import ctypes as C
import functools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import layout_ref as L
from test_gather_isa import FLAGS, HIPCC, function
from test_kmeans import engine_for, ring, spills

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu

# The restatement against scikit-learn's trustworthiness (float64 copies of the inputs) on the five inputs of SKLEARN_SHAPES, both
# directions, as measured with the restatement as committed: identical to the last bit in nine of the ten comparisons and 6.1e-8 in one
# (trustworthiness at (500, 64, 2, 90), penalty sum 161295: a near-tie that orders differently in fp32).  16 times the largest seen is
# allowed.
TRUST_TOL = 16 * 6.1e-8
# The restatement's PCA on the inputs of PCA_SHAPES: eigenvalues against numpy.linalg.eigvalsh of the restatement's own scatter matrix,
# relative to the largest eigenvalue, 2.34e-14, 2.38e-14, 1.23e-15, 1.55e-15, 1.32e-14; the projection (recomputed in fp64 from the
# returned mean and components, signs aligned) against scikit-learn's PCA(svd_solver="full") 3.06e-13, 2.77e-13, 3.46e-14, 5.77e-15,
# 1.01e-13.  16 times the largest seen is allowed; the returned fp32 projection may differ by half an fp32 ulp of its largest value more.
EIG_RTOL = 16 * 2.38e-14
PROJ_TOL = 16 * 3.06e-13
SKLEARN_SHAPES = [(300, 128, 2, 5), (257, 100, 3, 12), (400, 16, 2, 30), (200, 8, 2, 5), (500, 64, 2, 90)]
PCA_SHAPES = [(300, 128, 2), (257, 100, 3), (400, 16, 2), (1000, 64, 2), (300, 5, 2)]


def clustered(n, D, seed):
    """Rows are 6 centres x 2 plus unit noise: leading eigenvalues well apart."""
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((6, D))
    return (centres[rng.integers(0, 6, n)] + rng.standard_normal((n, D))).astype(np.float32)


def plain_layout(X, d2):
    """Any reasonable picture of X for the trustworthiness tests (numpy's SVD, fp32): the score takes every second matrix."""
    X64 = X.astype(np.float64)
    X64 = X64 - X64.mean(0)
    return (X64 @ np.linalg.svd(X64, full_matrices=False)[2][:d2].T).astype(np.float32)


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_null_and_bad_arguments():
    lib = _lib.lib()
    info, out = _lib.PcaInfo(), _lib.TrustInfo()
    y = np.zeros(8, dtype=np.float32)
    assert lib.f2v_pca(None, 2, None, None, None, None, C.byref(info)) == _lib.F2V_EINVAL
    assert b"f2v_pca" in lib.f2v_last_error() and b"null" in lib.f2v_last_error()
    assert lib.f2v_trustworthiness(None, y.ctypes.data_as(_lib.f32p), 2, 5, None, 0, None, None, C.byref(out)) == _lib.F2V_EINVAL
    assert b"f2v_trustworthiness" in lib.f2v_last_error() and b"null" in lib.f2v_last_error()
    assert (F.PCA_PIECE, F.TRUST_MAX_DIM) == (_lib.PCA_PIECE, _lib.TRUST_MAX_DIM) == (L.PIECE, 512) == (4096, 512)
    assert "f2v_pca" in _lib.SIGNATURES and "f2v_trustworthiness" in _lib.SIGNATURES and "f2v_test_pca_scatter" in _lib.TEST_SIGNATURES
    header = open(os.path.join(ROOT, "include", "f2v.h")).read()
    for line in ("#define F2V_PCA_PIECE 4096", "#define F2V_TRUST_MAX_DIM 512"):
        assert line in header, line
    assert C.sizeof(_lib.PcaInfo) == 24 and C.sizeof(_lib.TrustInfo) == 56


@pytest.mark.parametrize("args,word", [(["-layout", "-1"], "-layout"), (["-layout", "17", "-dim", "16"], "-layout"), (["-layout-neighbours", "0"], "-layout-neighbours"),
                                       (["-layout-neighbours", "129"], "-layout-neighbours"), (["-layout-sample", "-1"], "-layout-sample"),
                                       (["-layout", "2", "-gpus", "2"], "-layout")])
def test_cli_rejects_bad_layout_flags_before_reading_the_graph(tmp_path, args, word):
    for mtx in (os.path.join(tmp_path, "missing.mtx"), golden_graph_path("karate.mtx")):
        r = subprocess.run([CLI, "-input", mtx, "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1, r.stdout + r.stderr
        assert word in r.stdout and "Reading input" not in r.stdout, r.stdout
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


KERNELS = ["pca_colsum_kernel", "pca_reduce_kernel", "pca_scatter_kernel", "pca_project_kernel", "trust_keys_kernel", "trust_rank_kernelILi64EE",
           "trust_rank_kernelILi128EE", "trust_finish_kernel"]
TU = """#include "f2v_layout.hip.h"
template __global__ void f2v::trust_rank_kernel<64>(const f2v::TrustRankArgs);
template __global__ void f2v::trust_rank_kernel<128>(const f2v::TrustRankArgs);
"""


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "layout_isa.hip"), str(tmp_path / "layout_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


def test_restated_fma_equals_exact_arithmetic():
    """fma64 against the correctly rounded exact value, with cancelling addends among the cases."""
    rng = np.random.default_rng(5)
    a = rng.standard_normal(2000) * np.exp(rng.uniform(-20, 20, 2000))
    b = rng.standard_normal(2000) * np.exp(rng.uniform(-20, 20, 2000))
    c = -(a * b) * (1 + rng.standard_normal(2000) * np.array([0, 1e-16, 1e-10, 1])[rng.integers(0, 4, 2000)])
    c = c + rng.standard_normal(2000) * np.array([0, 1e-30, 1])[rng.integers(0, 3, 2000)]
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(L.fma64(a, b, c), want) and (a * b + c != want).sum() > 500  # ... which two roundings miss


def test_restated_sums_take_pieces_of_4096():
    """The restatement's mean and scatter chains against plain loops over pieces."""
    X = clustered(4096 + 200, 3, 9)
    sums = []
    for p in range(0, len(X), 4096):
        s = np.zeros(3)
        for row in X[p:p + 4096]:
            s = s + row.astype(np.float64)
        sums.append(s)
    m = (sums[0] + sums[1]) / float(len(X))
    assert len(sums) == 2 and np.array_equal(L.mean(X), m)
    Z = X.astype(np.float64) - m
    pieces = []
    for p in range(0, len(X), 4096):
        acc = Fraction(0)
        for z in Z[p:p + 4096]:
            acc = Fraction(float(Fraction(float(z[0])) * Fraction(float(z[2])) + acc))  # one rounding per fma
        pieces.append(float(acc))
    S = L.scatter(X)
    assert S[0, 2] == S[2, 0] == pieces[0] + pieces[1] and S[0, 2] != float((Z[:, 0] * Z[:, 2]).sum())


@pytest.mark.parametrize("n,D,d2,k", SKLEARN_SHAPES, ids=["n%d-D%d-d%d-k%d" % s for s in SKLEARN_SHAPES])
def test_restated_trustworthiness_agrees_with_scikit_learn(n, D, d2, k):
    manifold = pytest.importorskip("sklearn.manifold")
    X = clustered(n, D, 100 + n)
    Y = plain_layout(X, d2)
    got = L.trust(X, Y, k)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    tw, ct = manifold.trustworthiness(X64, Y64, n_neighbors=k), manifold.trustworthiness(Y64, X64, n_neighbors=k)
    print("n=%d D=%d d2=%d k=%d: trustworthiness %.17g (sklearn differs by %.3g, penalty %d), continuity %.17g (%.3g, penalty %d), overlap %.6f" % (
        n, D, d2, k, got.trustworthiness, abs(got.trustworthiness - tw), got.penalty_x, got.continuity, abs(got.continuity - ct), got.penalty_y, got.overlap))
    assert abs(got.trustworthiness - tw) <= TRUST_TOL and abs(got.continuity - ct) <= TRUST_TOL
    assert 0 < got.hits <= n * k and got.penalty_x == int(got.samples_x.sum()) and got.penalty_y == int(got.samples_y.sum())


@functools.lru_cache(maxsize=None)
def restated_pca(n, D, seed=None):
    """(X, mean, scatter, eigenvalues, V, sweeps, converged) of the clustered input: computed once, shared, never changed."""
    X = clustered(n, D, 100 + n if seed is None else seed)
    return (X,) + restated_eig(X)


def restated_eig(X):
    m = L.mean(X)
    S = L.scatter(X, m)
    return (m, S) + L.jacobi(S)


@pytest.mark.parametrize("n,D,d2", PCA_SHAPES, ids=["n%d-D%d-d%d" % s for s in PCA_SHAPES])
def test_restated_pca_agrees_with_numpy_and_scikit_learn(n, D, d2):
    decomposition = pytest.importorskip("sklearn.decomposition")
    X, m, S, lam, V, sweeps, converged = restated_pca(n, D)
    W, top = L.components(lam, V, d2)
    y = L.project(X, m, W)
    ev = np.linalg.eigvalsh(S)[::-1]
    X64 = X.astype(np.float64)
    ref = decomposition.PCA(n_components=d2, svd_solver="full").fit_transform(X64)
    sign = np.sign((ref * y.astype(np.float64)).sum(0))
    y64 = (X64 - m) @ W.T
    d_eig, d_proj, d_y = np.abs(np.sort(lam)[::-1] - ev).max() / ev[0], np.abs(y64 * sign - ref).max(), np.abs(y * sign - ref).max()
    print("n=%d D=%d d2=%d: %d sweeps, eigenvalues relative %.3g, projection %.3g (fp32 %.3g of %.3g)" % (n, D, d2, sweeps, d_eig, d_proj, d_y, np.abs(ref).max()))
    assert converged and sweeps <= 12 and d_eig <= EIG_RTOL and d_proj <= PROJ_TOL
    assert d_y <= PROJ_TOL + np.abs(ref).max() * 2.0 ** -24
    assert np.array_equal(top, np.sort(lam)[::-1][:d2]) and all(w[np.argmax(np.abs(w))] > 0 for w in W)
    assert np.allclose(W @ W.T, np.eye(d2), atol=1e-13)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_pca(got, X, m, S, lam, V, sweeps, converged, d2, name):
    W, top = L.components(lam, V, d2)
    n = len(X)
    print("%s d2=%d: sweeps %d/%d, mean differing %d, components differing %d, y differing %d" % (
        name, d2, got.info.sweeps, sweeps, int((bits(got.mean) != bits(m)).sum()), int((bits(got.components) != bits(W)).sum()),
        int((bits(got.y) != bits(L.project(X, m, W))).sum())))
    assert np.array_equal(bits(got.mean), bits(m))
    assert np.array_equal(bits(got.components), bits(W))
    assert np.array_equal(bits(got.variance), bits(top / float(n - 1)))
    assert got.info.sweeps == sweeps and got.info.converged == converged
    assert got.info.total_variance == float(L.K.seq_sum(np.diag(S))) / float(n - 1)
    assert np.array_equal(bits(got.y), bits(L.project(X, m, W)))


GPU_PCA = [(300, 128, (2,)), (4097, 20, (2,)), (8192 + 37, 5, (2,)), (130, 100, (1, 2, 3, 100))]


@gpu
@pytest.mark.parametrize("n,D,dims", GPU_PCA, ids=["n%d-D%d" % s[:2] for s in GPU_PCA])
def test_pca_equals_the_restatement_bit_for_bit(n, D, dims):
    parts = restated_pca(n, D)
    eng = engine_for(parts[0])
    try:
        for d2 in dims:
            got = eng.pca(d2, details=True)
            check_pca(got, *parts, d2, "n=%d D=%d" % (n, D))
            assert np.array_equal(bits(eng.pca(d2)), bits(got.y)) and eng.last_layout_seconds > 0
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("kind", ["constant column", "rank one"])
def test_pca_of_a_degenerate_matrix_equals_the_restatement(kind):
    rng = np.random.default_rng(11)
    if kind == "constant column":
        X = clustered(200, 12, 3)
        X[:, 3] = np.float32(1.25)  # a zero row and column of the scatter matrix: a zero eigenvalue
    else:
        X = np.outer(rng.standard_normal(150), rng.standard_normal(10)).astype(np.float32)
    parts = restated_eig(X)
    eng = engine_for(X)
    try:
        for d2 in (2, X.shape[1]):
            check_pca(eng.pca(d2, details=True), X, *parts, d2, kind)
    finally:
        eng.close()
    lam = np.sort(parts[2])[::-1]
    assert (np.abs(lam) < 1e-9 * lam[0]).sum() >= (1 if kind == "constant column" else 9)


@gpu
def test_scatter_at_dimension_512_equals_the_restatement():
    """36 tiles of 64 x 64 entries, 8 of them on the diagonal; the eigen-solver is left out (its restatement would take minutes)."""
    X = clustered(257, 512, 77)
    rowptr, colids = ring(257)
    eng = F.Engine(rowptr, colids, 512, selftest=True)
    try:
        eng.set_embeddings(X)
        m, S = np.empty(512), np.empty((512, 512))
        eng._ck(eng._L.f2v_test_pca_scatter(eng._h, m.ctypes.data_as(_lib.f64p), S.ctypes.data_as(_lib.f64p)))
    finally:
        eng.close()
    want_m = L.mean(X)
    want = L.scatter(X, want_m)
    print("D=512: mean differing %d, scatter entries differing %d" % (int((bits(m) != bits(want_m)).sum()), int((bits(S) != bits(want)).sum())))
    assert np.array_equal(bits(m), bits(want_m)) and np.array_equal(bits(S), bits(want))


def same_trust(got, want, samples=True):
    ok = (got.penalty_x == want.penalty_x and got.penalty_y == want.penalty_y and got.hits == want.hits and got.trustworthiness == want.trustworthiness and
          got.continuity == want.continuity and got.overlap == want.overlap)
    return ok and (not samples or (np.array_equal(got.samples_x, want.samples_x) and np.array_equal(got.samples_y, want.samples_y)))


def report(name, got, want):
    print("%s: trustworthiness %.17g/%.17g continuity %.17g/%.17g hits %d/%d, samples differing %d + %d" % (
        name, got.trustworthiness, want.trustworthiness, got.continuity, want.continuity, got.hits, want.hits,
        int((got.samples_x != want.samples_x).sum()), int((got.samples_y != want.samples_y).sum())))


TRUST_SHAPES = SKLEARN_SHAPES + [(130, 5, 2, 5), (130, 512, 2, 5), (300, 16, 1, 5), (200, 8, 2, 1), (40, 8, 2, 19), (300, 16, 2, 128)]


@gpu
@pytest.mark.parametrize("n,D,d2,k", TRUST_SHAPES, ids=["n%d-D%d-d%d-k%d" % s for s in TRUST_SHAPES])
def test_trustworthiness_equals_the_restatement_bit_for_bit(n, D, d2, k):
    X = clustered(n, D, 100 + n)
    Y = plain_layout(X, d2)
    eng = engine_for(X)
    try:
        got = eng.trustworthiness(Y, k, samples=True)
        assert same_trust(eng.trustworthiness(Y, k), got, samples=False) and eng.last_layout_seconds > 0
    finally:
        eng.close()
    want = L.trust(X, Y, k)
    report("n=%d D=%d d2=%d k=%d" % (n, D, d2, k), got, want)
    assert same_trust(got, want)


@gpu
def test_a_sample_subset_is_ranked_against_all_vertices():
    """n = 4096 + 300: the candidates of a sample block span 18 workgroups.  64 seeded samples in the restatement, every vertex on
    the GPU."""
    n, D, k = 4096 + 300, 16, 7
    X = clustered(n, D, 21)
    Y = plain_layout(X, 2)
    ids = np.random.default_rng(2).permutation(n)[:64]
    eng = engine_for(X)
    try:
        sub, full = eng.trustworthiness(Y, k, ids, samples=True), eng.trustworthiness(Y, k, samples=True)
    finally:
        eng.close()
    want = L.trust(X, Y, k, ids)
    report("n=%d subset" % n, sub, want)
    assert same_trust(sub, want)
    assert np.array_equal(full.samples_x[ids], want.samples_x) and np.array_equal(full.samples_y[ids], want.samples_y) and len(full.samples_x) == n


@gpu
def test_ties_resolve_by_id_and_a_nan_ranks_last():
    n, D, k = 300, 8, 6
    X = clustered(n, D, 31)
    X[100:170] = X[100]  # 70 identical rows: a tie group longer than a sweep of 64 candidates
    X[7] = X[250]
    Y = plain_layout(X, 2)
    Y[20:24] = Y[20]
    Y[200] = Y[3]
    X[17, 3] = np.nan  # every distance to vertex 17 is a NaN: it is the last of every other vertex's order
    ids = np.array([250, 250, 170, 169, 100, 17, 7, 3, 3], dtype=np.uint32)  # duplicates, descending
    eng = engine_for(X)
    try:
        full, sub = eng.trustworthiness(Y, k, samples=True), eng.trustworthiness(Y, k, ids, samples=True)
    finally:
        eng.close()
    want, want_sub = L.trust(X, Y, k), L.trust(X, Y, k, ids)
    report("ties", full, want)
    assert same_trust(full, want) and same_trust(sub, want_sub)
    assert np.array_equal(sub.samples_x, full.samples_x[ids]) and np.array_equal(sub.samples_y, full.samples_y[ids])
    places = L.places(X, np.array([0, 100, 299]))
    assert (places[:, 17] == n - 1).all() and places[1, 101] == 1 and places[1, 169] == 69


@gpu
def test_identities():
    n, D, k = 257, 24, 9
    X = clustered(n, D, 41)
    Y = plain_layout(X, 3)
    perm = np.random.default_rng(4).permutation(n)
    a = engine_for(X)
    b = engine_for(Y)
    try:
        same = a.trustworthiness(X, k, samples=True)
        assert same.trustworthiness == 1.0 and same.continuity == 1.0 and same.overlap == 1.0 and same.hits == n * k
        assert same.penalty_x == same.penalty_y == 0 and not same.samples_x.any() and not same.samples_y.any()
        mixed = a.trustworthiness(X[perm], k, samples=True)
        want = L.trust(X, X[perm], k)
        report("rows permuted", mixed, want)
        assert same_trust(mixed, want) and mixed.trustworthiness < 0.8 and mixed.continuity < 0.8
        fwd, back = a.trustworthiness(Y, k, samples=True), b.trustworthiness(X, k, samples=True)  # the roles swapped: D = 3, d2 = 24
        assert fwd.trustworthiness == back.continuity and fwd.continuity == back.trustworthiness and fwd.overlap == back.overlap
        assert np.array_equal(fwd.samples_x, back.samples_y) and np.array_equal(fwd.samples_y, back.samples_x)
    finally:
        a.close()
        b.close()


@gpu
def test_results_do_not_depend_on_calls_handles_or_tunables():
    n, D, k = 700, 40, 5
    X = clustered(n, D, 51)
    Y = plain_layout(X, 2)
    ids = np.random.default_rng(3).permutation(n)[:300]
    eng = engine_for(X)

    def run(e):
        p = e.pca(2, details=True)
        return p, e.trustworthiness(Y, k, samples=True), e.trustworthiness(p.y, k, ids, samples=True)

    def same(x, y):
        return (all(np.array_equal(bits(p), bits(q)) for p, q in zip(x[0][:4], y[0][:4])) and x[0].info[2:] == y[0].info[2:] and
                same_trust(x[1], y[1]) and same_trust(x[2], y[2]))

    try:
        base = run(eng)
        assert same(run(eng), base)
        other = engine_for(X)
        try:
            assert same(run(other), base), "second handle"
        finally:
            other.close()
        for name, values, default in (("trust_chunk", (64, 100, 8192), 8192), ("trust_block", (64, 128, 0), 0), ("nearest_chunk", (50, 8192), 8192),
                                      ("nearest_splits", (1, 3, 0), 0), ("nearest_block", (32, 128, 0), 0)):
            for v in values:
                eng.set_param(name, v)
                assert eng.get_param(name) == v and same(run(eng), base), (name, v)
            eng.set_param(name, default)
        eng.set_param("trust_chunk", 100)
        eng.set_param("trust_block", 128)
        assert same(run(eng), base)
        eng.set_param("trust_chunk", 8192)
        eng.set_param("trust_block", 0)
        eng.kmeans(9, 3, seed=2)
        eng.nearest(ids=np.arange(50), k=12, metric="cos")  # shares the nearest-neighbour workspace
        eng.silhouette(np.arange(n) % 4)
        assert same(run(eng), base), "after other evaluation calls"
        wide = eng.trustworthiness(np.hstack([Y, np.zeros((n, 298), dtype=np.float32)]), k, samples=True)  # d2 = 300 > D: the dimensions past 2 are zeros
        assert same_trust(wide, base[1]) and same(run(eng), base)
        for name, bad in (("trust_block", 32), ("trust_block", 256), ("trust_chunk", 0)):
            with pytest.raises(F.F2VError) as e:
                eng.set_param(name, bad)
            assert e.value.code == _lib.F2V_EINVAL and name in str(e.value)
    finally:
        eng.close()


@gpu
def test_scoring_does_not_change_training_and_sees_pending_rows():
    rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))
    n = len(rowptr) - 1

    def run(score):
        eng = F.Engine(rowptr, colids, 16)
        try:
            eng.srand(1)
            eng.init_embeddings(0)
            eng.train(5, 3, 16, 5, 0.02)
            if score:
                eng.trustworthiness(eng.pca(2), 5, samples=True)
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
        eng.minibatch_step(5, 0, n // 2, ids, 5, 0.02)  # a partial range pending: the calls see what get_embeddings returns
        got = eng.pca(2, details=True)
        score = eng.trustworthiness(got.y, 5, samples=True)
        X = eng.get_embeddings()
    finally:
        eng.close()
    check_pca(got, X, *restated_eig(X), 2, "karate, pending rows")
    assert same_trust(score, L.trust(X, got.y, 5))


@gpu
def test_every_error_case_is_refused_and_training_goes_on():
    rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 16)
    try:
        lib, h = eng._L, eng._h
        info, out = _lib.PcaInfo(), _lib.TrustInfo()
        Y = np.random.default_rng(0).random((n, 2), dtype=np.float32)
        u32 = lambda a: a.ctypes.data_as(_lib.u32p)

        def pca(d2=2, info=info):
            return lib.f2v_pca(h, d2, None, None, None, None, C.byref(info) if info is not None else None)

        def trust(Y=Y, d2=2, k=5, ids=None, nq=0, out=out):
            return lib.f2v_trustworthiness(h, Y.ctypes.data_as(_lib.f32p) if Y is not None else None, d2, k, u32(ids) if ids is not None else None, nq, None, None,
                                           C.byref(out) if out is not None else None)

        assert pca() == trust() == _lib.F2V_ESTATE  # before init_embeddings
        eng.srand(1)
        eng.init_embeddings(0)
        # (n < 2 cannot be reached: f2v_create refuses such a graph)
        cases = [("pca: null info", lambda: pca(info=None)), ("pca: d2 = 0", lambda: pca(d2=0)), ("pca: d2 > D", lambda: pca(d2=17)),
                 ("null Y", lambda: trust(Y=None)), ("null out", lambda: trust(out=None)), ("d2 = 0", lambda: trust(d2=0)), ("d2 = 513", lambda: trust(d2=513)),
                 ("k = 0", lambda: trust(k=0)), ("k = 129", lambda: trust(k=129)), ("2 k = n", lambda: trust(k=n // 2)),
                 ("a sample id >= n", lambda: trust(ids=np.array([1, n], dtype=np.uint32), nq=2)),
                 ("nq = 0 with sample ids", lambda: trust(ids=np.array([1], dtype=np.uint32), nq=0))]
        for name, call in cases:
            lib.f2v_set_param(h, b"no_such_param", 0)  # leaves another message behind
            before = lib.f2v_last_error()
            assert call() == _lib.F2V_EINVAL, name
            msg = lib.f2v_last_error()
            assert msg and msg != before and (b"f2v_pca" in msg or b"f2v_trustworthiness" in msg), (name, msg)
        assert pca(d2=16) == _lib.F2V_OK and trust(k=n // 2 - 1) == _lib.F2V_OK and trust(ids=np.array([2, 2], dtype=np.uint32), nq=2) == _lib.F2V_OK
        with pytest.raises(ValueError):
            eng.trustworthiness(Y[:-1])
        eng.train(5, 2, 16, 5, 0.02)
        X = eng.get_embeddings()
        assert np.isfinite(X).all() and same_trust(eng.trustworthiness(Y, 5, samples=True), L.trust(X, Y, 5))
    finally:
        eng.close()


@gpu
def test_cora_layout_equals_the_restatement_and_scikit_learn():
    """Option 5, 200 epochs at batch 256 and D = 32 from srand(1).  No quality level is asserted: nobody has measured one.  The
    restatement scores 100 seeded samples, scikit-learn every vertex."""
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    n = len(rowptr) - 1
    ids = np.random.default_rng(6).permutation(n)[:100]
    eng = F.Engine(rowptr, colids, 32)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        eng.train(5, 200, 256, 5, 0.02)
        X = eng.get_embeddings()
        p = eng.pca(2, details=True)
        t_pca = eng.last_layout_seconds
        full, sub = eng.trustworthiness(p.y, 5, samples=True), eng.trustworthiness(p.y, 5, ids, samples=True)
        print("cora: pca %.3f ms (%d sweeps, explained %.4f), trustworthiness %.17g continuity %.17g overlap %.4f (%.3f ms for %d samples)" % (
            t_pca * 1e3, p.info.sweeps, p.variance.sum() / p.info.total_variance, full.trustworthiness, full.continuity, full.overlap, full.seconds * 1e3, n))
    finally:
        eng.close()
    check_pca(p, X, *restated_eig(X), 2, "cora")
    want = L.trust(X, p.y, 5, ids)
    assert same_trust(sub, want) and np.array_equal(full.samples_x[ids], want.samples_x) and np.array_equal(full.samples_y[ids], want.samples_y)
    try:
        from sklearn import manifold
    except ImportError:
        return
    X64, Y64 = X.astype(np.float64), p.y.astype(np.float64)
    tw, ct = manifold.trustworthiness(X64, Y64, n_neighbors=5), manifold.trustworthiness(Y64, X64, n_neighbors=5)
    print("cora against scikit-learn: trustworthiness differs by %.3g, continuity by %.3g" % (abs(full.trustworthiness - tw), abs(full.continuity - ct)))
    assert abs(full.trustworthiness - tw) <= TRUST_TOL and abs(full.continuity - ct) <= TRUST_TOL


@gpu
def test_cli_writes_the_layout_and_prints_its_scores(tmp_path):
    mtx = golden_graph_path("cora.mtx")
    r = subprocess.run([CLI, "-input", mtx, "-iter", "5", "-dim", "32", "-batch", "256", "-option", "5", "-binout", "1", "-layout", "2", "-layout-sample", "200",
                        "-output", str(tmp_path) + "/"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^TrustWorthiness: (\S+) Continuity: (\S+)$", r.stdout, re.M)
    m2 = re.search(r"^Layout: d=2 neighbours=5 samples=200 :EXPLAINED-VARIANCE: (\S+) :OVERLAP: (\S+) :SWEEPS: (\d+)$", r.stdout, re.M)
    assert m and m2, r.stdout
    embd = [p for p in os.listdir(tmp_path) if p.endswith(".embd")]
    assert len(embd) == 1
    rows = [line.split() for line in open(str(tmp_path / embd[0]) + ".lay").read().splitlines()]
    rowptr, colids = F.read_mtx(mtx)
    n = len(rowptr) - 1
    assert len(rows) == n and [int(t[0]) for t in rows] == list(range(1, n + 1)) and all(len(t) == 3 for t in rows)
    eng = F.Engine(rowptr, colids, 32)
    try:
        eng.set_embeddings(F.read_embd_bin(str(tmp_path / embd[0]) + ".bin", n, 32))
        p = eng.pca(2, details=True)
        keys = L.K.mix64(L.K.mix64(np.uint64(1)) ^ np.arange(n, dtype=np.uint64))
        ids = np.lexsort((np.arange(n), keys))[:200]
        t = eng.trustworthiness(p.y, 5, ids)
    finally:
        eng.close()
    assert [[float("%g" % v) for v in row] for row in p.y] == [[float(v) for v in t[1:]] for t in rows]
    assert float(m.group(1)) == t.trustworthiness and float(m.group(2)) == t.continuity and float(m2.group(2)) == t.overlap
    assert float(m2.group(1)) == p.variance.sum() / p.info.total_variance and int(m2.group(3)) == p.info.sweeps
