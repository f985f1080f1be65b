"""GPU k-means clustering of the embedding matrix and graph modularity (include/f2v.h: f2v_kmeans, f2v_modularity; Engine.kmeans /
Engine.modularity; the CLI's -cluster).

Host tests (no GPU): argument checks, the exported constants, the CLI's refusals before the graph is read, and the compiled gfx950
code of every kernel of f2v_kmeans.hip.h (no scratch, nothing spilled, both builds).  -m gpu: labels, centroids, counts, inertia and
iteration count bit for bit against the numpy restatement of the definition (tests/kmeans_ref.py); given centroids, duplicates, an
empty cluster and a NaN row; restarts; independence of calls, handles and tunables; non-interference with training; the modularity
tallies against the restatement and tests/cluster_harness.py; the clustering quality of a trained cora embedding against the
reference's own table; the CLI's .clu file."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import kmeans_ref as K
from test_gather_isa import FLAGS, HIPCC, function

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_null_and_bad_arguments():
    L = _lib.lib()
    labels = np.zeros(8, dtype=np.uint32)
    info, q = _lib.KMeansInfo(), C.c_double()
    lp = labels.ctypes.data_as(_lib.u32p)
    assert L.f2v_kmeans(None, 2, 10, 1, 1, None, lp, None, None, C.byref(info)) == _lib.F2V_EINVAL
    assert L.f2v_modularity(None, lp, 2, C.byref(q), None, None, None) == _lib.F2V_EINVAL
    assert b"null" in L.f2v_last_error()
    assert (F.KMEANS_MAX_K, F.KMEANS_PIECE) == (1024, 64) and (_lib.KMEANS_MAX_K, _lib.KMEANS_PIECE) == (1024, 64)
    assert C.sizeof(_lib.KMeansInfo) == 32
    assert "f2v_kmeans" in _lib.SIGNATURES and "f2v_modularity" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "f2v.h")).read()
    assert "#define F2V_KMEANS_MAX_K 1024" in header and "#define F2V_KMEANS_PIECE 64" in header


@pytest.mark.parametrize("args,word", [(["-cluster", "-1"], "-cluster"), (["-cluster", "1025"], "-cluster"),
                                       (["-cluster", "4", "-cluster-restarts", "0"], "-cluster-restarts"),
                                       (["-cluster", "4", "-gpus", "2"], "-cluster")])
def test_cli_rejects_bad_cluster_flags_before_reading_the_graph(tmp_path, args, word):
    for mtx in (os.path.join(tmp_path, "missing.mtx"), golden_graph_path("karate.mtx")):
        r = subprocess.run([CLI, "-input", mtx, "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1, r.stdout + r.stderr
        assert word in r.stdout and "Reading input" not in r.stdout, r.stdout
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


KERNELS = ["kmeans_assign_kernelILi64EE", "kmeans_assign_kernelILi128EE", "kmeans_assign_kernelILi256EE", "kmeans_hist_kernel",
           "kmeans_offsets_kernel", "kmeans_starts_kernel", "kmeans_scatter_kernel", "kmeans_piece_sum_kernel", "kmeans_centroid_kernel",
           "kmeans_inertia_piece_kernel", "kmeans_inertia_reduce_kernel", "modularity_kernel"]
TU = """#include "f2v_kmeans.hip.h"
template __global__ void f2v::kmeans_assign_kernel<64>(const f2v::KmAssignArgs);
template __global__ void f2v::kmeans_assign_kernel<128>(const f2v::KmAssignArgs);
template __global__ void f2v::kmeans_assign_kernel<256>(const f2v::KmAssignArgs);
"""


def spills(text, symbol):
    """-> the kernel's spill and scratch figures from the compiler's metadata (SGPR spills go to VGPR lanes: still spills)."""
    for entry in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):]):
        if re.search(r"\.name:\s+%s\s*\n" % re.escape(symbol), entry):
            return {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry)}
    raise AssertionError("no metadata for " + symbol)


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "kmeans_isa.hip"), str(tmp_path / "kmeans_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


def test_restated_seed_rows_and_sums():
    """The restatement's own pieces: mix64 against the splitmix64 reference value, distinct seeded rows, sequential piece sums."""
    assert int(K.mix64(np.uint64(0))) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    rows = K.seed_rows(1000, 50, 7)
    assert len(set(rows.tolist())) == 50 and not np.array_equal(rows, K.seed_rows(1000, 50, 8)[:50])
    a = np.random.default_rng(0).standard_normal(200)
    want = 0.0
    parts = []
    for p in range(0, 200, 64):
        s = 0.0
        for x in a[p:p + 64]:
            s += x
        parts.append(s)
    for s in parts:
        want += s
    assert K.piece_sum(a) == want


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def ring(n):
    """A ring of n vertices: rowptr, colids (ascending inside every row)."""
    v = np.arange(n)
    nb = np.sort(np.stack([(v - 1) % n, (v + 1) % n], axis=1), axis=1)
    return (2 * np.arange(n + 1)).astype(np.uint32), nb.reshape(-1).astype(np.uint32)


def engine_for(X):
    n, D = X.shape
    if n == 34:
        rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))
    else:
        rowptr, colids = ring(n)
    eng = F.Engine(rowptr, colids, D)
    eng.set_embeddings(X)
    return eng


def blobs(n, D, k, seed):
    rng = np.random.default_rng(seed)
    centres = (3.0 * rng.standard_normal((k, D))).astype(np.float32)
    return (centres[rng.integers(0, k, n)] + 0.5 * rng.standard_normal((n, D))).astype(np.float32)


def noise(n, D, k, seed):
    return np.random.default_rng(seed).random((n, D), dtype=np.float32)


SHAPES = [(300, 128, 7, 10), (1000, 16, 3, 50), (257, 100, 3, 5), (130, 5, 2, 5), (200, 512, 4, 3), (2100, 64, 130, 4)]


@gpu
@pytest.mark.parametrize("data", [blobs, noise], ids=["blobs", "noise"])
@pytest.mark.parametrize("n,D,k,iters", SHAPES, ids=["n%d-D%d-K%d-it%d" % s for s in SHAPES])
def test_results_equal_the_restatement_bit_for_bit(n, D, k, iters, data):
    X = data(n, D, k, 1000 + n)
    eng = engine_for(X)
    try:
        got = eng.kmeans(k, iters, seed=3)
    finally:
        eng.close()
    want = K.kmeans(X, k, iters, seed=3)
    print("n=%d D=%d K=%d: iterations %d/%d converged %s/%s inertia %.17g/%.17g labels differing %d" % (
        n, D, k, got.iterations, want.iterations, got.converged, want.converged, got.inertia, want.inertia, int((got.labels != want.labels).sum())))
    assert np.array_equal(got.labels, want.labels)
    assert np.array_equal(got.centroids.view(np.uint32), want.centroids.view(np.uint32))
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == n
    assert got.inertia == want.inertia and got.iterations == want.iterations and got.converged == want.converged
    if (n, data) == (1000, noise):
        assert got.converged and 1 < got.iterations < iters and got.counts.min() > 4 * 64  # five or six pieces per cluster, run to convergence


TILED = [  # n, D, k, iters, kmeans_block values: shapes whose centroids do not fit the resident 64 KiB, or whose workgroup asks for more than 64 KiB of LDS
    (1200, 128, 200, 2, (0, 64, 128, 256)),  # tiles of 128 centroids and a partial last tile of 72 (one whole sweep and a partial one at 64 rows)
    (700, 512, 70, 2, (0, 64, 128, 256)),    # one sweep per tile at 64 rows (64 + 6 centroids, 141 KiB of LDS), tiles of 32 at 128 / 256 rows
    (600, 128, 120, 2, (256,)),              # resident centroids (60 KiB) beside a 256-row stage: 100 KiB, the raised dynamic-LDS limit without tiling
]


@gpu
@pytest.mark.parametrize("n,D,k,iters,blocks", TILED, ids=["n%d-D%d-K%d" % s[:3] for s in TILED])
def test_tiled_centroids_and_large_lds_equal_the_restatement(n, D, k, iters, blocks):
    """kmeans_assign_kernel keeps at most 16384 centroid values (64 KiB) in LDS: beyond that the centroids pass in tiles of whole
    sweeps with a partial last tile, and a launch may ask for more than the 64 KiB of dynamic LDS a kernel gets by default."""
    X = blobs(n, D, max(k // 4, 2), 2000 + n)
    want = K.kmeans(X, k, iters, seed=9)
    assert k * ((D + 31) // 32 * 32) > 16384 or blocks == (256,)
    eng = engine_for(X)
    try:
        for block in blocks:
            eng.set_param("kmeans_block", block)
            got = eng.kmeans(k, iters, seed=9)
            print("n=%d D=%d K=%d kmeans_block=%d: iterations %d/%d inertia %.17g/%.17g labels differing %d" % (
                n, D, k, block, got.iterations, want.iterations, got.inertia, want.inertia, int((got.labels != want.labels).sum())))
            assert K.same(got, want), (block, int((got.labels != want.labels).sum()))
        assert int(want.counts.sum()) == n and len(np.unique(want.labels)) > k // 8  # labels from every tile, not only the first
        assert want.labels.max() >= min(k - 1, 128) or blocks == (256,)
    finally:
        eng.close()


@gpu
def test_given_centroids_duplicates_empty_cluster_and_nan():
    rng = np.random.default_rng(4)
    D = 16
    centres = np.zeros((3, D), dtype=np.float32)
    centres[1, 0], centres[2, 1] = 40.0, 40.0
    X = (centres[rng.integers(0, 3, 34)] + 0.5 * rng.standard_normal((34, D))).astype(np.float32)
    C0 = np.stack([centres[0], centres[1] + 2.0, centres[2], centres[1] + 2.0]).astype(np.float32)  # rows 1 and 3 are one point, off the blob's centre
    eng = engine_for(X)
    try:
        got = eng.kmeans(4, 0, init=C0)
        want = K.kmeans(X, 4, 0, init=C0)
        assert K.same(got, want) and got.iterations == 0 and not got.converged
        assert np.array_equal(got.centroids.view(np.uint32), C0.view(np.uint32))
        assert got.counts[1] > 0 and got.counts[3] == 0 and not (got.labels == 3).any()  # the lower index takes all of their rows
        one = eng.kmeans(4, 1, init=C0)
        assert K.same(one, K.kmeans(X, 4, 1, init=C0)) and one.iterations == 1
        assert np.array_equal(one.centroids[3].view(np.uint32), C0[3].view(np.uint32)) and one.counts[3] == 0  # the empty one: unchanged
        assert not np.array_equal(one.centroids[1], C0[1])
        assert np.array_equal(one.labels, K.assign(X, one.centroids)[0])  # labels == assign(X, centroids)
        Xn = X.copy()
        Xn[7] = np.nan  # every distance of the row is NaN: label 0
        eng.set_embeddings(Xn)
        got = eng.kmeans(4, 0, init=C0)
        want = K.kmeans(Xn, 4, 0, init=C0)
        assert got.labels[7] == 0 and np.array_equal(got.labels, want.labels) and np.isnan(got.inertia) and np.isnan(want.inertia)
    finally:
        eng.close()


@gpu
def test_restarts_keep_the_run_of_lowest_inertia():
    X = noise(400, 32, 6, 21)
    eng = engine_for(X)
    try:
        singles = [eng.kmeans(6, 20, seed=s) for s in (5, 6, 7)]
        got = eng.kmeans(6, 20, seed=5, restarts=3)
        assert len({s.inertia for s in singles}) == 3
        r = int(np.argmin([s.inertia for s in singles]))
        assert got.restart == r and K.same(got, singles[r]._replace(restart=r))
        assert K.same(got, K.kmeans(X, 6, 20, seed=5, restarts=3))
        with pytest.raises(F.F2VError) as e:
            eng.kmeans(6, 20, restarts=2, init=X[:6])
        assert e.value.code == _lib.F2V_EINVAL
    finally:
        eng.close()


@gpu
def test_results_do_not_depend_on_calls_handles_or_tunables():
    X = blobs(700, 64, 5, 33)
    eng = engine_for(X)
    try:
        base = {k: eng.kmeans(k, 5, seed=2) for k in (2, 3, 70)}
        for k, want in base.items():
            assert K.same(eng.kmeans(k, 5, seed=2), want), k
        other = engine_for(X)
        try:
            for k, want in base.items():
                assert K.same(other.kmeans(k, 5, seed=2), want), ("second handle", k)
        finally:
            other.close()
        for name, values, default in (("kmeans_block", (64, 128, 256, 0), 0), ("waves_per_block", (1, 2, 4), None), ("rows_in_flight", (4, 8, 0), 0)):
            default = eng.get_param(name) if default is None else default
            for v in values:
                eng.set_param(name, v)
                for k, want in base.items():
                    assert K.same(eng.kmeans(k, 5, seed=2), want), (name, v, k)
            eng.set_param(name, default)
        with pytest.raises(F.F2VError) as e:
            eng.set_param("kmeans_block", 32)
        assert e.value.code == _lib.F2V_EINVAL and "kmeans_block must be 0, 64, 128 or 256" in str(e.value)
    finally:
        eng.close()


@gpu
def test_clustering_does_not_change_training_and_sees_pending_rows():
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    n = len(rowptr) - 1

    def run(query):
        eng = F.Engine(rowptr, colids, 128)
        try:
            eng.srand(1)
            eng.init_embeddings(0)
            eng.train(5, 1, 256, 5, 0.02)
            if query:
                res = eng.kmeans(7, 3, seed=1, restarts=2)
                eng.modularity(res.labels, 7)
            eng.train(5, 1, 256, 5, 0.02)
            return eng.get_embeddings(), eng.rand_index(1 << 30)
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1]
    eng = F.Engine(rowptr, colids, 128)
    try:
        L, h = eng._L, eng._h
        labels = np.zeros(n, dtype=np.uint32)
        info = _lib.KMeansInfo()
        call = lambda k=4, restarts=1, init=None: L.f2v_kmeans(h, k, 2, restarts, 1, init, labels.ctypes.data_as(_lib.u32p), None, None, C.byref(info))
        assert call() == _lib.F2V_ESTATE  # before init_embeddings
        eng.srand(1)
        eng.init_embeddings(0)
        assert call(k=0) == call(k=1025) == call(restarts=0) == _lib.F2V_EINVAL
        assert L.f2v_kmeans(h, 4, 2, 1, 1, None, None, None, None, C.byref(info)) == _lib.F2V_EINVAL
        assert L.f2v_kmeans(h, 4, 2, 1, 1, None, labels.ctypes.data_as(_lib.u32p), None, None, None) == _lib.F2V_EINVAL
        ids = eng.draw_samples(n - 1, 5)
        eng.minibatch_step(5, 0, n // 2, ids, 5, 0.02)  # a partial range pending: k-means sees what get_embeddings returns
        got = eng.kmeans(4, 2, seed=1)
        X = eng.get_embeddings()
        assert K.same(got, K.kmeans(X, 4, 2, seed=1)) and eng.last_kmeans_seconds > 0
    finally:
        eng.close()
    small = F.Engine(*ring(5), 8)
    try:
        small.set_embeddings(np.zeros((5, 8), dtype=np.float32))
        with pytest.raises(F.F2VError) as e:
            small.kmeans(6)  # k > n
        assert e.value.code == _lib.F2V_EINVAL
    finally:
        small.close()


HAND = (np.array([0, 4, 5, 6, 6, 8, 9], dtype=np.uint32), np.array([0, 1, 1, 2, 0, 3, 5, 5, 4], dtype=np.uint32))  # edges 00 01 02 23 45


def graph(name):
    return HAND if name == "hand" else F.read_mtx(golden_graph_path(name + ".mtx"))


@gpu
@pytest.mark.parametrize("name", ["karate", "cora", "hand"])
def test_modularity_tallies_are_exact(name):
    import cluster_harness as CH
    rowptr, colids = graph(name)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 8)  # no embeddings needed
    try:
        rng = np.random.default_rng(6)
        for nc in (1, 4, n):
            labels = rng.integers(0, nc, n).astype(np.uint32)
            got = eng.modularity(labels, nc)
            edges, inside, degree = K.tallies(rowptr, colids, labels, nc)
            assert got.edges == edges and np.array_equal(got.inside, inside) and np.array_equal(got.degree, degree), (name, nc)
            assert got.q == K.modularity_q(edges, inside, degree), (name, nc)
            assert abs(got.q - CH.modularity(rowptr, colids, labels)) <= 1e-12, (name, nc)
            assert int(got.degree.sum()) == 2 * got.edges
            if nc == 1:
                assert got.q == 0.0  # one community
        assert eng.modularity(np.zeros(n, dtype=np.uint32)).q == 0.0  # n_clusters from the labels
        if name == "hand":
            assert eng.modularity(np.zeros(n, dtype=np.uint32)).edges == 5
        if name == "cora":
            assert eng.modularity(np.zeros(n, dtype=np.uint32)).edges == (int(rowptr[-1]) - 302) // 2  # 302 duplicate entries collapse
        with pytest.raises(F.F2VError) as e:
            eng.modularity(np.full(n, 4, dtype=np.uint32), 4)  # a label >= n_clusters
        assert e.value.code == _lib.F2V_EINVAL
    finally:
        eng.close()
    if name == "karate":
        shuffled = colids.copy()
        shuffled[rowptr[0]:rowptr[1]] = shuffled[rowptr[0]:rowptr[1]][::-1]  # row 0 descending: a row search would miss neighbours
        eng = F.Engine(rowptr, shuffled, 8)
        try:
            with pytest.raises(F.F2VError) as e:
                eng.modularity(np.zeros(n, dtype=np.uint32))
            assert e.value.code == _lib.F2V_EINVAL and "ascending" in str(e.value)
        finally:
            eng.close()


@gpu
def test_cora_clusters_level_with_the_reference_scorer():
    """Option 5, 1200 epochs at batch 256 from srand(1) (the run of test_gpu_parity's clustering gate), kmeans(k, restarts=10, seed=1)
    and modularity on the GPU for k in (7, 10, 16, 25) against the table of the reference's OWN embedding under its own scorer
    (manifest modularity_reference_cora_opt5_it1200_B256_D128): every count >= table - 0.03, the best of the four >= the table's best
    of the four - 0.02.  Basis (CPU, this definition on the reference-order embedding, seeds 1..10, lowest inertia): 0.7312 / 0.7639 /
    0.7875 / 0.8006 against 0.7408 / 0.7712 / 0.7865 / 0.7991 -- worst deficit 0.0096; the kernels' summation order moves modularity by
    <= 0.006 (test_gpu_parity.py); the margin is about twice the sum of the two."""
    with open(os.path.join(GOLD, "manifest.json")) as f:
        ref = {int(k): v for k, v in json.load(f)["modularity_reference_cora_opt5_it1200_B256_D128"]["table"].items()}
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    eng = F.Engine(rowptr, colids, 128)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        eng.train(5, 1200, 256, 5, 0.02)
        got = {}
        for k in (7, 10, 16, 25):
            res = eng.kmeans(k, restarts=10, seed=1)
            got[k] = eng.modularity(res.labels, k).q
            print("cora k=%d: modularity %.4f (table %.4f), inertia %.6g, %d iterations, restart %d, %.3f ms" % (
                k, got[k], ref[k], res.inertia, res.iterations, res.restart, eng.last_kmeans_seconds * 1e3))
    finally:
        eng.close()
    for k in got:
        assert got[k] >= ref[k] - 0.03, (k, got[k], ref[k])
    assert max(got.values()) >= max(ref[k] for k in got) - 0.02, (got, ref)


@gpu
def test_cli_writes_the_clu_file(tmp_path):
    mtx = golden_graph_path("karate.mtx")
    r = subprocess.run([CLI, "-input", mtx, "-iter", "3", "-dim", "16", "-batch", "16", "-option", "5", "-binout", "1", "-cluster", "4",
                        "-output", str(tmp_path) + "/"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    embd = [p for p in os.listdir(tmp_path) if p.endswith(".embd")]
    assert len(embd) == 1
    rowptr, colids = F.read_mtx(mtx)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 16)
    try:
        eng.set_embeddings(F.read_embd_bin(str(tmp_path / embd[0]) + ".bin", n, 16))
        res = eng.kmeans(4, 300, seed=1, restarts=10)
        q = eng.modularity(res.labels, 4).q
    finally:
        eng.close()
    lines = open(str(tmp_path / embd[0]) + ".clu").read().splitlines()
    assert [int(x.split()[0]) for x in lines] == list(range(n))
    assert np.array_equal(np.array([int(x.split()[1]) for x in lines], dtype=np.uint32), res.labels)
    m = re.search(r"Clusters:4 :MODULARITY: (\S+) :INERTIA: (\S+) :ITERATIONS: (\d+) :RESTART: (\d+)", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)) == q and float(m.group(2)) == res.inertia and (int(m.group(3)), int(m.group(4))) == (res.iterations, res.restart)
