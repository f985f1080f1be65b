"""Deterministic t-SNE layout of the embedding on the GPU (include/f2v.h: f2v_tsne_affinities, f2v_tsne, f2v_tsne_kl_log; Engine.tsne /
Engine.tsne_affinities; the CLI's -layout-method tsne).

Host tests (no GPU): the numpy restatement of the definition (tests/tsne_ref.py) is sane -- conditional rows, entropies, the symmetric
P -- and good: on eight Gaussian blobs its layout is as trustworthy as scikit-learn's exact t-SNE and far better than a PCA layout;
the C surface, the CLI's help and refusals, the compiled gfx950 code of every kernel of f2v_tsne.hip.h (no scratch, nothing spilled).
-m gpu: the device's P against the restatement (structure identical, values to the tolerance recorded in
tests/golden/tsne_manifest.json: exp and log are the device library's); the iteration bit for bit from the device's own P, the KL log
and Z included; independence of tunables, handles and calls; a subset against an engine of its rows; non-interference with training; the
PCA start; the quality bars on the device; every refusal; the CLI.

Figures behind the recorded numbers (tests/golden/tsne_manifest.json): on the blobs scikit-learn's TSNE(2, perplexity=30, init="pca",
method="exact", random_state=0) reaches a trustworthiness (k = 5) of 0.98008, the restatement's fast mode 0.97926, a PCA layout 0.88658."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import tsne_ref as T
from test_gather_isa import FLAGS, HIPCC, function
from test_kmeans import engine_for, spills

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "tsne_manifest.json")))
# (m, D, perplexity) of the affinity cases; the third holds two identical rows and a far outlier that nobody lists as a neighbour
AFFINITY_CASES = [(70, 8, 5.0), (300, 16, 30.0), (1100, 16, 30.0)]


@functools.lru_cache(maxsize=None)
def points(m, D):
    X = np.random.default_rng(100 + m).standard_normal((m, D)).astype(np.float32)
    if m == 1100:
        X[900] = X[17]
        X[500] = 1000.0 + X[500]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def restated_affinities(m, D, perplexity):
    return T.affinities(points(m, D), perplexity)


@functools.lru_cache(maxsize=None)
def device_affinities(m, D, perplexity):
    """The device's own P of a case (what both sides of the bit-for-bit tests start from)."""
    eng = engine_for(np.array(points(m, D)))
    try:
        return eng.tsne_affinities(perplexity)
    finally:
        eng.close()


def start(m, d2):
    return 1e-4 * np.random.default_rng(7 * m + d2).standard_normal((m, d2))


# ---- host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,D,perplexity", AFFINITY_CASES[:2] + [(600, 32, 30.0)])
def test_restated_affinities_are_sane(m, D, perplexity):
    X = T.blobs() if m == 600 else points(m, D)
    k = int(3 * perplexity)
    ids, d = T.neighbours(X, k)
    cond, H = T.conditionals(d, perplexity)
    assert ids.shape == cond.shape == (m, k) and (d >= 0).all() and (np.diff(d, axis=1) >= 0).all()
    assert np.abs(cond.sum(1) - 1.0).max() <= 1e-12 and np.abs(H - np.log(perplexity)).max() <= 1e-5
    rowptr, colids, values = T.symmetric(ids, cond)
    assert rowptr[0] == 0 and rowptr[-1] == len(colids) == len(values) <= 2 * m * k and abs(values.sum() - 1.0) <= 1e-12
    dense = np.zeros((m, m))
    for i in range(m):
        row = colids[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(row.astype(np.int64)) > 0).all() and i not in row and set(ids[i]) <= set(row)
        dense[i, row] = values[rowptr[i]:rowptr[i + 1]]
    assert np.array_equal(dense, dense.T) and (values >= T.TINY).all()


def test_restated_modes_agree_and_the_log_follows_the_iterations():
    m = 70
    P, y0 = restated_affinities(m, 8, 5.0), start(m, 2)
    a = T.run(P, y0, iters=12, exaggeration_iters=8, kl_every=4, exact=True)
    b = T.run(P, y0, iters=12, exaggeration_iters=8, kl_every=4, exact=False)
    assert list(a.kl_iters) == [4, 8, 12] and a.kl == a.kl_values[-1] and a.learning_rate == 50.0
    # the modes differ in the fp32 piece sums alone: 64 positive terms added in fp32 are off by at most 63 half-ulps relative to their sum
    assert abs(a.z - b.z) <= 64 * 2.0 ** -24 * a.z and abs(a.kl - b.kl) <= 1e-5 and np.abs(a.y - b.y).max() <= 1e-4 * np.abs(a.y).max()
    c = T.run(P, np.hstack([y0, start(m, 3)[:, :1]]), iters=3, exact=True)
    assert c.y.shape == (m, 3) and np.isfinite(c.y).all()


def test_the_definition_lays_out_blobs_as_well_as_scikit_learn():
    """The fast-mode restatement, default parameters, on the blobs: trustworthiness (k = 5) at least scikit-learn's exact t-SNE minus
    0.02 (the margin covers the kNN-truncated P and the fixed iteration count against its dense P and stopping rule) and at least a PCA
    layout's plus 0.05.  Measured: scikit-learn 0.98008, the restatement 0.97926, PCA 0.88658."""
    manifold = pytest.importorskip("sklearn.manifold")
    from sklearn.decomposition import PCA

    X = T.blobs()
    X64 = X.astype(np.float64)
    pca = PCA(2, svd_solver="full").fit(X64)
    proj = pca.transform(X64).astype(np.float32)
    got = T.run(T.affinities(X, 30.0), T.pca_start(proj, pca.explained_variance_[0]), exact=False, kl_every=300)
    sk = manifold.TSNE(2, perplexity=30, init="pca", method="exact", random_state=0).fit_transform(X)
    t_ref, t_got, t_pca = (manifold.trustworthiness(X, Y, n_neighbors=5) for Y in (sk, got.y, proj))
    print("blobs: trustworthiness scikit-learn %.5f restatement %.5f PCA %.5f; KL %.5f at 300, %.5f at the end" % (t_ref, t_got, t_pca, got.kl_values[0], got.kl))
    assert abs(t_ref - MANIFEST["sklearn_trustworthiness"]) <= 0.005 and abs(t_pca - MANIFEST["pca_trustworthiness"]) <= 0.005
    assert t_got >= t_ref - 0.02 and t_got >= t_pca + 0.05
    assert got.kl < got.kl_values[0]


def test_surface_of_the_c_abi():
    lib = _lib.lib()
    for name in ("f2v_tsne_affinities", "f2v_tsne", "f2v_tsne_kl_log"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "f2v.h")).read()
    for line in ("#define F2V_TSNE_PIECE 64", "#define F2V_TSNE_SPAN 16", "F2V_API int f2v_tsne(", "F2V_API int f2v_tsne_affinities("):
        assert line in header, line
    assert (F.TSNE_PIECE, F.TSNE_SPAN) == (T.PIECE, T.SPAN) == (64, 16)
    assert C.sizeof(_lib.TsneParams) == 40 and C.sizeof(_lib.TsneInfo) == 48
    info, count = _lib.TsneInfo(), C.c_uint32()
    y = np.zeros(16, dtype=np.float32)
    assert lib.f2v_tsne(None, None, 8, 2, None, None, None, None, None, y.ctypes.data_as(_lib.f32p), C.byref(info)) == _lib.F2V_EINVAL
    assert b"f2v_tsne" in lib.f2v_last_error() and b"null" in lib.f2v_last_error()
    assert lib.f2v_tsne_kl_log(None, None, None, 0, C.byref(count)) == _lib.F2V_EINVAL


def test_cli_lists_and_checks_the_layout_method(tmp_path):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, cwd=tmp_path)
    for flag in ("-layout-method", "-layout-perplexity", "-layout-iters"):
        assert flag in r.stdout, flag
    for args, word in ((["-layout", "4", "-layout-method", "tsne"], "2 or 3"), (["-layout", "2", "-layout-method", "umap"], "pca or tsne"),
                       (["-layout", "2", "-layout-method", "tsne", "-layout-perplexity", "1"], "-layout-perplexity"),
                       (["-layout", "2", "-layout-method", "tsne", "-layout-iters", "0"], "-layout-iters")):
        for mtx in (os.path.join(tmp_path, "missing.mtx"), golden_graph_path("karate.mtx")):
            r = subprocess.run([CLI, "-input", mtx, "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
            assert r.returncode == 1 and word in r.stdout and "Reading input" not in r.stdout, r.stdout + r.stderr
    # more vertices than the CLI lays out: refused when the graph has been read, with the way out named
    big = tmp_path / "big.mtx"
    with open(big, "w") as f:
        f.write("%%MatrixMarket matrix coordinate pattern symmetric\n131073 131073 131072\n")
        f.write("".join("%d %d\n" % (v + 1, v) for v in range(1, 131073)))
    r = subprocess.run([CLI, "-input", str(big), "-iter", "1", "-dim", "16", "-layout", "2", "-layout-method", "tsne"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 2 and "Engine.tsne(ids=...)" in r.stderr and "131072" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


KERNELS = ["tsne_pair_kernelILi2ELi64EE", "tsne_pair_kernelILi2ELi128EE", "tsne_pair_kernelILi2ELi256EE", "tsne_pair_kernelILi3ELi64EE",
           "tsne_pair_kernelILi3ELi128EE", "tsne_pair_kernelILi3ELi256EE", "tsne_step_kernelILi2EE", "tsne_step_kernelILi3EE", "tsne_kl_kernelILi2EE",
           "tsne_kl_kernelILi3EE", "tsne_zpiece_kernel", "tsne_seqsum_kernel", "tsne_calibrate_kernel"]
TU = '#include "f2v_tsne.hip.h"\n' + "".join(
    "template __global__ void f2v::tsne_pair_kernel<%d, %d>(const f2v::TsnePairArgs);\n" % (d, r) for d in (2, 3) for r in (64, 128, 256)) + "".join(
    "template __global__ void f2v::tsne_step_kernel<%d>(const f2v::TsneStepArgs);\ntemplate __global__ void f2v::tsne_kl_kernel<%d>(const f2v::TsneKlArgs);\n" % (d, d)
    for d in (2, 3))


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "tsne_isa.hip"), str(tmp_path / "tsne_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, body = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))
        if "tsne_pair_kernel" in part:  # pair arithmetic is separate roundings: the only fused operations are the division's own
            assert "v_div_fixup_f32" in body and "v_pk_fma_f32" not in body, symbol


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m,D,perplexity", AFFINITY_CASES)
def test_affinities_equal_the_restatement(m, D, perplexity):
    """Structure identical; values within 16 x the largest relative difference measured against the restatement (manifest:
    "affinity_rel_err"; 4.44e-16, 6.66e-16 and 5.55e-16 in the three cases), which is itself below 1e-9: only the last places of exp and
    log differ between host and device."""
    got, want = device_affinities(m, D, perplexity), restated_affinities(m, D, perplexity)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    err = float(np.abs(got[2] / want[2] - 1.0).max())
    print("affinities (%d, %d, %g): %d entries, largest relative difference %.3g" % (m, D, perplexity, len(got[1]), err))
    recorded = MANIFEST["affinity_rel_err"]
    assert recorded < 1e-9 and err <= 16 * recorded
    if m == 1100:  # nobody lists the outlier: its row holds (those that are left of) its own 90 neighbours alone; the twins list each other
        assert 1 <= got[0][501] - got[0][500] <= 90 and 900 in got[1][got[0][17]:got[0][18]] and 17 in got[1][got[0][900]:got[0][901]]


ITERATION_CASES = [(64, 8, 5.0, 2, 20, 250, 0), (70, 8, 5.0, 2, 20, 250, 0), (1100, 16, 30.0, 2, 5, 250, 0), (1100, 16, 30.0, 3, 5, 250, 0),
                   (300, 16, 30.0, 2, 300, 250, 50)]


@gpu
@pytest.mark.parametrize("m,D,perplexity,d2,iters,ex_iters,kl_every", ITERATION_CASES)
def test_iteration_is_bit_for_bit_the_restatement(m, D, perplexity, d2, iters, ex_iters, kl_every):
    """One piece exactly (64), a partial second piece (70), across a span with a partial last piece and identical rows (1100: a = 0,
    w = 1), and 300 iterations across the exaggeration and momentum switch with the KL log.  Both sides start from the device's P."""
    P, y0 = device_affinities(m, D, perplexity), start(m, d2)
    eng = engine_for(np.array(points(m, D)))
    try:
        y, info = eng.tsne(d2, iters=iters, P=P, init=y0, exaggeration_iters=ex_iters, kl_every=kl_every, details=True)
    finally:
        eng.close()
    want = T.run(P, y0, iters=iters, exaggeration_iters=ex_iters, kl_every=kl_every, exact=True)
    print("iteration (%d, %d, %d): largest |y| %.3g, differing coordinates %d, KL %.17g / %.17g, Z %.17g / %.17g" % (
        m, d2, iters, np.abs(want.y).max(), int((y != want.y).sum()), info["kl"], want.kl, info["z"], want.z))
    assert np.array_equal(y, want.y)
    assert info["kl"] == want.kl and info["z"] == want.z and info["learning_rate"] == want.learning_rate and info["nnz"] == len(P[1]) and info["k"] == 0
    assert np.array_equal(info["kl_iters"], want.kl_iters) and np.array_equal(info["kl_values"], want.kl_values)
    if kl_every:
        assert list(info["kl_iters"]) == list(range(kl_every, iters + 1, kl_every))


@gpu
def test_bits_do_not_depend_on_placement_handles_or_calls():
    m, D, perplexity = 1100, 16, 30.0
    P, y0 = device_affinities(m, D, perplexity), start(m, 2)
    X = np.array(points(m, D))
    eng, other = engine_for(X), engine_for(X)
    try:
        base = eng.tsne(2, iters=4, P=P, init=y0, kl_every=2, details=True)
        for rows, slices in ((64, 1), (128, 2), (256, 1), (256, 0), (0, 2)):
            eng.set_param("tsne_rows", rows)
            eng.set_param("tsne_slices", slices)
            got = eng.tsne(2, iters=4, P=P, init=y0, kl_every=2, details=True)
            assert np.array_equal(got[0], base[0]) and got[1]["kl"] == base[1]["kl"] and got[1]["z"] == base[1]["z"], (rows, slices)
            assert np.array_equal(got[1]["kl_values"], base[1]["kl_values"])
        eng.set_param("tsne_rows", 0)
        eng.set_param("tsne_slices", 0)
        assert eng.get_param("tsne_rows") == 0 and eng.get_param("tsne_slices") == 0
        for name, bad in (("tsne_rows", 32), ("tsne_rows", 512), ("tsne_slices", -1)):
            with pytest.raises(F.F2VError):
                eng.set_param(name, bad)
        again, theirs = eng.tsne(2, iters=4, P=P, init=y0), other.tsne(2, iters=4, P=P, init=y0)
        assert np.array_equal(again, base[0]) and np.array_equal(theirs, base[0])
        # P computed by the call itself is the P of tsne_affinities; the PCA start is the start handed in as `init`
        own = eng.tsne(2, perplexity=perplexity, iters=4, init=y0)
        assert np.array_equal(own, base[0])
        p = eng.pca(2, details=True)
        a = eng.tsne(2, perplexity=perplexity, iters=4)
        b = eng.tsne(2, iters=4, P=P, init=T.pca_start(p.y, p.variance[0]))
        assert np.array_equal(a, b) and np.isfinite(a).all()
        # a shuffled subset is laid out as an engine that holds only those rows would be
        ids = np.random.default_rng(3).permutation(m)[:300].astype(np.uint32)
        sub = engine_for(X[ids])
        try:
            Ps, Pi = sub.tsne_affinities(10.0), eng.tsne_affinities(10.0, ids=ids)
            assert all(np.array_equal(x, y) for x, y in zip(Ps, Pi))
            assert np.array_equal(sub.tsne(3, perplexity=10.0, iters=6, init=start(300, 3)), eng.tsne(3, perplexity=10.0, iters=6, ids=ids, init=start(300, 3)))
        finally:
            sub.close()
    finally:
        eng.close()
        other.close()


@gpu
def test_layout_does_not_change_training():
    rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))

    def run(layout):
        eng = F.Engine(rowptr, colids, 16)
        try:
            eng.srand(1)
            eng.init_embeddings(0)
            eng.train(5, 3, 16, 5, 0.02)
            before = eng.get_embeddings()
            if layout:
                eng.tsne_affinities(5.0)
                eng.tsne(2, perplexity=5.0, iters=10, kl_every=5, details=True)
                assert np.array_equal(eng.get_embeddings().view(np.uint32), before.view(np.uint32))
            draw = eng.rand_index(1 << 30)
            eng.train(5, 5, 16, 5, 0.02)
            return eng.get_embeddings(), draw, eng.rand_index(1 << 30)
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1:] == b[1:]


@gpu
def test_device_layout_of_the_blobs_meets_the_quality_bars():
    """Defaults on the blobs: Engine.trustworthiness(Y, k = 5) at least scikit-learn's recorded 0.98008 minus 0.02 and at least the PCA
    layout's plus 0.05; the divergence at the end is below the one at iteration 300."""
    X = T.blobs()
    eng = engine_for(X)
    try:
        y, info = eng.tsne(2, kl_every=300, details=True)
        t_got, t_pca = eng.trustworthiness(y, 5).trustworthiness, eng.trustworthiness(eng.pca(2), 5).trustworthiness
    finally:
        eng.close()
    print("blobs on the device: trustworthiness %.5f (PCA %.5f), KL %.5f at 300, %.5f at the end, %.3f s, %d nonzeros" % (
        t_got, t_pca, info["kl_values"][0], info["kl"], info["seconds"], info["nnz"]))
    assert y.shape == (600, 2) and np.isfinite(y).all() and info["k"] == 90 and info["learning_rate"] == 50.0
    assert list(info["kl_iters"]) == [300, 600, 900]
    assert t_got >= MANIFEST["sklearn_trustworthiness"] - 0.02 and t_got >= t_pca + 0.05
    assert info["kl"] < info["kl_values"][0]


@gpu
def test_every_refusal_and_training_goes_on():
    rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 16)
    try:
        lib, h = eng._L, eng._h
        u32 = lambda a: a.ctypes.data_as(_lib.u32p) if a is not None else None  # noqa: E731
        f64 = lambda a: a.ctypes.data_as(_lib.f64p) if a is not None else None  # noqa: E731
        info, nnz = _lib.TsneInfo(), C.c_uint64()
        y = np.zeros((n, 3), dtype=np.float32)
        rp, ci, va = np.zeros(n + 1, dtype=np.uint32), np.zeros(2 * n * 15, dtype=np.uint32), np.zeros(2 * n * 15, dtype=np.float64)

        def aff(ids=None, m=n, perplexity=5.0, rp=rp, ci=ci, va=va, cap=len(ci), nnz=nnz):
            return lib.f2v_tsne_affinities(h, u32(ids), m, perplexity, u32(rp), u32(ci), f64(va), cap, C.byref(nnz) if nnz is not None else None, None)

        def tsne(ids=None, m=n, d2=2, P=(None, None, None), init=None, y=y, info=info, **par):
            p = _lib.TsneParams(par.get("perplexity", 5.0), par.get("exaggeration", 0.0), par.get("learning_rate", 0.0), par.get("iters", 3), 0, 0, 0)
            return lib.f2v_tsne(h, u32(ids), m, d2, C.byref(p), u32(P[0]), u32(P[1]), f64(P[2]), f64(init), y.ctypes.data_as(_lib.f32p) if y is not None else None,
                                C.byref(info) if info is not None else None)

        assert aff() == tsne() == _lib.F2V_ESTATE  # before init_embeddings
        eng.srand(1)
        eng.init_embeddings(0)
        assert aff() == _lib.F2V_OK
        good = (rp.copy(), ci[: nnz.value].copy(), va[: nnz.value].copy())
        assert tsne(P=good) == _lib.F2V_OK
        descending, reaching, partial, negative = [tuple(a.copy() for a in good) for _ in range(4)]
        descending[1][:2] = descending[1][1::-1]
        reaching[1][good[0][1] - 1] = n
        negative[2][3] = -negative[2][3]
        dup = np.arange(n, dtype=np.uint32)
        dup[5] = 4
        zeros = np.zeros((n, 16), dtype=np.float32)
        cases = [("null y_out", lambda: tsne(y=None)), ("null info", lambda: tsne(info=None)), ("null nnz_out", lambda: aff(nnz=None)),
                 ("null rowptr_out", lambda: aff(rp=None)), ("null colids_out", lambda: aff(ci=None)), ("null values_out", lambda: aff(va=None)),
                 ("d2 = 1", lambda: tsne(d2=1)), ("d2 = 4", lambda: tsne(d2=4)),
                 ("m < 8", lambda: tsne(ids=np.arange(7, dtype=np.uint32), m=7, perplexity=2.0)), ("m < 8", lambda: aff(ids=np.arange(7, dtype=np.uint32), m=7, perplexity=2.0)),
                 ("a sample id >= n", lambda: tsne(ids=np.arange(1, n + 1, dtype=np.uint32))), ("a sample id >= n", lambda: aff(ids=np.arange(1, n + 1, dtype=np.uint32))),
                 ("a duplicate sample id", lambda: tsne(ids=dup)), ("a duplicate sample id", lambda: aff(ids=dup)),
                 ("perplexity = 1", lambda: tsne(perplexity=1.0)), ("perplexity = 1", lambda: aff(perplexity=1.0)), ("perplexity NaN", lambda: tsne(perplexity=float("nan"))),
                 ("perplexity NaN", lambda: aff(perplexity=float("nan"))), ("perplexity < 0", lambda: tsne(perplexity=-3.0)),
                 ("k > 128", lambda: tsne(perplexity=43.0)), ("k > 128", lambda: aff(perplexity=43.0)),
                 ("k >= m", lambda: tsne(perplexity=11.4)), ("k >= m", lambda: aff(perplexity=11.4)),
                 ("P in part", lambda: tsne(P=(good[0], good[1], None))), ("P in part", lambda: tsne(P=(None, good[1], good[2]))),
                 ("P descends", lambda: tsne(P=descending)), ("P reaches m", lambda: tsne(P=reaching)), ("P negative", lambda: tsne(P=negative)),
                 ("cap too small", lambda: aff(cap=nnz.value - 1)), ("a negative exaggeration", lambda: tsne(exaggeration=-1.0)),
                 ("a NaN learning rate", lambda: tsne(learning_rate=float("nan")))]
        for name, call in cases:
            lib.f2v_set_param(h, b"no_such_param", 0)  # leaves another message behind
            before = lib.f2v_last_error()
            assert call() == _lib.F2V_EINVAL, name
            msg = lib.f2v_last_error()
            assert msg and msg != before and b"f2v_tsne" in msg, (name, msg)
        count = nnz.value
        assert aff(cap=count - 1) == _lib.F2V_EINVAL and nnz.value == count  # nnz_out still answers
        assert tsne(perplexity=11.3) == _lib.F2V_OK and info.k == 33 and aff(cap=count) == _lib.F2V_OK
        with pytest.raises(ValueError):
            eng.tsne(2, P=good, init=np.zeros((n, 3)))
        with pytest.raises(ValueError):
            eng.tsne(2, P=(good[0][:-1], good[1], good[2]))
        eng.set_embeddings(zeros)  # a matrix without variance has no PCA start, but takes one that is given
        assert tsne(P=good) == _lib.F2V_EINVAL and b"variance" in lib.f2v_last_error()
        assert tsne(P=good, init=start(n, 2)) == _lib.F2V_OK
        eng.srand(1)
        eng.init_embeddings(0)
        eng.train(5, 2, 16, 5, 0.02)
        assert np.isfinite(eng.get_embeddings()).all() and np.isfinite(eng.tsne(3, perplexity=5, iters=5)).all()
    finally:
        eng.close()


@gpu
def test_cli_writes_the_tsne_layout_and_keeps_the_pca_layout(tmp_path):
    """karate has 34 vertices: the default perplexity of 30 asks for 90 neighbours and is refused, so the run names a perplexity of 5."""
    mtx = golden_graph_path("karate.mtx")
    common = [CLI, "-input", mtx, "-iter", "20", "-dim", "16", "-batch", "16", "-option", "5", "-binout", "1", "-layout", "2"]
    out = {}
    for name, extra in (("tsne", ["-layout-method", "tsne", "-layout-iters", "300", "-layout-perplexity", "5"]), ("pca", []), ("pca2", ["-layout-method", "pca"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(common + extra + ["-output", str(d) + "/"], capture_output=True, text=True, cwd=d, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lay = [p for p in os.listdir(d) if p.endswith(".lay")]
        assert len(lay) == 1
        out[name] = (r.stdout, open(str(d / lay[0])).read(), str(d / lay[0]))
    assert out["pca"][1] == out["pca2"][1] and ":EXPLAINED-VARIANCE:" in out["pca"][0] and ":METHOD: tsne" not in out["pca"][0]
    stdout, text, path = out["tsne"]
    m = re.search(r"^TrustWorthiness: (\S+) Continuity: (\S+)$", stdout, re.M)
    m2 = re.search(r"^Layout: d=2 neighbours=5 samples=34 :METHOD: tsne :PERPLEXITY: 5 :ITERATIONS: 300 :KL: (\S+) :OVERLAP: (\S+)$", stdout, re.M)
    assert m and m2, stdout
    rows = [line.split() for line in text.splitlines()]
    assert len(rows) == 34 and [int(t[0]) for t in rows] == list(range(1, 35)) and all(len(t) == 3 for t in rows)
    assert text != out["pca"][1]
    rowptr, colids = F.read_mtx(mtx)
    eng = F.Engine(rowptr, colids, 16)
    try:
        eng.set_embeddings(F.read_embd_bin(path[: -len(".lay")] + ".bin", 34, 16))
        y, info = eng.tsne(2, perplexity=5, iters=300, details=True)
        t = eng.trustworthiness(y, 5)
    finally:
        eng.close()
    assert [[float("%g" % v) for v in row] for row in y] == [[float(v) for v in t[1:]] for t in rows]
    assert float(m.group(1)) == t.trustworthiness and float(m.group(2)) == t.continuity and float(m2.group(1)) == info["kl"] and float(m2.group(2)) == t.overlap
