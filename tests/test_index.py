"""Nearest neighbours through an inverted-file index (include/f2v.h, "nearest neighbours through an index": f2v_index_build /
_build_given / _get / _drop / _search_rows / _search_vectors; Engine.build_index / index / drop_index / index_search / index_recall;
the CLI's -nearest-lists).

Host tests (no GPU): argument checks, the constants, the CLI's refusals before the graph is read, the restatement against brute force,
and the compiled gfx950 code of the scan kernel, both instantiations, both builds: no scratch, nothing spilled.  -m gpu: every
comparison is array_equal -- an index search is exact top-k over a well-defined candidate set, and with every list probed it IS the
exact search."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import index_ref as I
import nearest_ref as R
from test_gather_isa import FLAGS, HIPCC, function
from test_kmeans import engine_for, spills

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu
METRICS = ("dot", "l2", "cos")
PAD = 0xFFFFFFFF


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_null_arguments_and_constants():
    L = _lib.lib()
    u32, f32 = _lib.u32p, _lib.f32p
    ids, out = np.zeros(4, dtype=np.uint32), np.zeros(40, dtype=np.uint32)
    cen = np.zeros(8, dtype=np.float32)
    assert L.f2v_index_build(None, 2, 5, 1, None, None) == _lib.F2V_EINVAL and b"null" in L.f2v_last_error()
    assert L.f2v_index_build_given(None, ids.ctypes.data_as(u32), cen.ctypes.data_as(f32), 2, None) == _lib.F2V_EINVAL
    assert L.f2v_index_get(None, None, None, None, None) == _lib.F2V_EINVAL
    assert L.f2v_index_drop(None) == _lib.F2V_EINVAL
    assert L.f2v_index_search_rows(None, ids.ctypes.data_as(u32), 4, 10, 0, 0, 8, out.ctypes.data_as(u32), None, None, None) == _lib.F2V_EINVAL
    assert L.f2v_index_search_vectors(None, cen.ctypes.data_as(f32), 1, 10, 0, 8, out.ctypes.data_as(u32), None, None, None) == _lib.F2V_EINVAL
    assert b"null" in L.f2v_last_error()
    assert (F.INDEX_MAX_LISTS, F.INDEX_MAX_PROBES) == (1024, 128) == (F.KMEANS_MAX_K, F.NEAREST_MAX_K)
    assert (_lib.INDEX_MAX_LISTS, _lib.INDEX_MAX_PROBES) == (1024, 128)
    assert C.sizeof(_lib.IndexInfo) == 48 and C.sizeof(_lib.IndexSearchInfo) == 24
    header = open(os.path.join(ROOT, "include", "f2v.h")).read()
    assert "#define F2V_INDEX_MAX_LISTS 1024" in header and "#define F2V_INDEX_MAX_PROBES 128" in header
    hpp = open(os.path.join(ROOT, "force2vec_amd", "csrc", "algorithms.hpp")).read()
    assert "kIndexMaxLists = F2V_INDEX_MAX_LISTS" in hpp and "kIndexMaxProbes = F2V_INDEX_MAX_PROBES" in hpp


@pytest.mark.parametrize("args,word", [(["-nearest", "5", "-nearest-lists", "1025"], "-nearest-lists"), (["-nearest", "5", "-nearest-lists", "-1"], "-nearest-lists"),
                                       (["-nearest", "5", "-nearest-lists", "8", "-nearest-probes", "129"], "-nearest-probes"),
                                       (["-nearest-lists", "8"], "-nearest"), (["-nearest-probes", "4"], "-nearest"),
                                       (["-nearest-check", "10"], "-nearest"), (["-nearest", "5", "-nearest-probes", "4"], "-nearest-lists")])
def test_cli_rejects_bad_index_flags_before_reading_the_graph(tmp_path, args, word):
    for mtx in (os.path.join(tmp_path, "missing.mtx"), golden_graph_path("karate.mtx")):
        r = subprocess.run([CLI, "-input", mtx, "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1, r.stdout + r.stderr
        assert word in r.stdout and "Reading input" not in r.stdout, r.stdout
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


def test_restatement_against_brute_force():
    """On a tiny case the restatement is checked against loops that know nothing of nearest_ref's ranking code."""
    rng = np.random.default_rng(5)
    n, D, lists = 40, 6, 5
    X = rng.integers(-3, 4, (n, D)).astype(np.float32)  # small integers: every chain is exact, many ties
    labels = rng.integers(0, lists - 1, n)              # the last list stays empty
    cen = rng.integers(-3, 4, (lists, D)).astype(np.float32)
    qids = np.arange(0, n, 3)
    for nprobe in (1, 2, 5, 9):
        ids, sc, pr, cand = I.index_ref(X, labels, cen, 4, "dot", nprobe, qids=qids, exclude_self=True)
        P = min(nprobe, lists)
        total = 0
        for i, v in enumerate(qids):
            order = sorted(range(lists), key=lambda c: (-float(X[v] @ cen[c]), c))[:P]
            assert pr[i].tolist() == order
            members = [u for u in range(n) if labels[u] in order]
            total += len(members)
            best = sorted((u for u in members if u != v), key=lambda u: (-float(X[v] @ X[u]), u))[:4]
            assert ids[i].tolist() == best + [PAD] * (4 - len(best))
            assert sc[i].tolist() == [float(X[v] @ X[u]) for u in best] + [-np.inf] * (4 - len(best))
        assert cand == total
    full = I.index_ref(X, labels, cen, 4, "l2", lists, qids=qids, exclude_self=True)
    assert R.same(full[:2], R.nearest_ref(X, 4, "l2", qids=qids, exclude_self=True))


KERNELS = ["index_scan_kernelILb0ELi1ELi1ELi1EE", "index_scan_kernelILb1ELi1ELi1ELi1EE", "index_scan_kernelILb0ELi2ELi2ELi2EE",
           "index_scan_kernelILb1ELi2ELi2ELi2EE", "index_count_kernel", "index_fill_kernel"]  # all that are launched
TU = """#include "f2v_index.hip.h"
template __global__ void f2v::index_scan_kernel<false, 1, 1, 1>(const f2v::IxArgs);
template __global__ void f2v::index_scan_kernel<true, 1, 1, 1>(const f2v::IxArgs);
template __global__ void f2v::index_scan_kernel<false, 2, 2, 2>(const f2v::IxArgs);
template __global__ void f2v::index_scan_kernel<true, 2, 2, 2>(const f2v::IxArgs);
"""


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "index_isa.hip"), str(tmp_path / "index_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, body = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))
        assert not re.search(r"\bscratch_(load|store)", body)
    for dot, l2, steps in ((KERNELS[0], KERNELS[1], 16), (KERNELS[2], KERNELS[3], 64)):
        assert len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", function(text, dot)[1])) >= steps  # one chunk of 32 dimensions: the exact search's chain
        assert not re.search(r"\bv_mfma", function(text, l2)[1])


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def clustered(n, D, centres, seed, spread=0.4):
    rng = np.random.default_rng(seed)
    C0 = (2.0 * rng.standard_normal((centres, D))).astype(np.float32)
    return (C0[rng.integers(0, centres, n)] + spread * rng.standard_normal((n, D))).astype(np.float32)


def cora_engine(D, seed=11):
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    eng = F.Engine(rowptr, colids, D)
    eng.set_embeddings(clustered(len(rowptr) - 1, D, 12, seed))
    return eng, rowptr, colids


def equal(got, want):
    """ids and scores agree bit for bit (up to the sign of a zero score and the payload of a NaN, as nearest_ref.same)"""
    return R.same(got[:2], want[:2])


@gpu
@pytest.mark.parametrize("lists", [1, 7, 40])
def test_exhaustive_probing_is_the_exact_search(lists):
    eng, rowptr, colids = cora_engine(64)
    try:
        n = eng.n
        info = eng.build_index(lists=lists, max_iters=5, seed=3)
        assert info.lists == lists
        vec = clustered(50, 64, 12, 99)
        for metric in METRICS:
            exact_v = eng.nearest(vectors=vec, k=10, metric=metric)
            exact = {f: eng.nearest(k=10, metric=metric, exclude_self=f[0], exclude_neighbours=f[1]) for f in ((False, False), (True, False), (True, True))}
            for nprobe in (lists, 128):
                for f, want in exact.items():
                    got = eng.index_search(k=10, metric=metric, nprobe=nprobe, exclude_self=f[0], exclude_neighbours=f[1], details=True)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True), (metric, nprobe, f)
                    assert got[3]["nprobe"] == lists and got[3]["candidates"] == n * n and got[2].shape == (n, lists)
                got = eng.index_search(vectors=vec, k=10, metric=metric, nprobe=nprobe)
                assert np.array_equal(got[0], exact_v[0]) and np.array_equal(got[1], exact_v[1]), (metric, nprobe, "vectors")
    finally:
        eng.close()


SIZES = [0, 1, 31, 32, 33, 127, 128, 129, 300]  # the tile (128) and sub-tile (32) boundaries of the scan kernel; one more list takes the rest
N_GIVEN = 1300


def given_partition(n, D, seed):
    """-> (labels, centroids): lists of the SIZES in a random arrangement of the vertices, random centroids (any values are legal)."""
    rng = np.random.default_rng(seed)
    sizes = SIZES + [n - sum(SIZES)]
    labels = np.empty(n, dtype=np.uint32)
    labels[rng.permutation(n)] = np.repeat(np.arange(len(sizes)), sizes)
    return labels, rng.standard_normal((len(sizes), D)).astype(np.float32)


@gpu
@pytest.mark.parametrize("D", [3, 40, 64, 128, 160])
@pytest.mark.parametrize("metric", METRICS)
def test_results_equal_the_restatement(D, metric):
    X = clustered(N_GIVEN, D, 9, D)
    labels, cen = given_partition(N_GIVEN, D, D + 1)
    eng = engine_for(X)
    try:
        info = eng.build_index(labels=labels, centroids=cen)
        assert (info.lists, info.largest, info.empty) == (10, N_GIVEN - sum(SIZES), 1) and (info.iterations, info.inertia) == (0, 0.0)
        lab, c2, counts = eng.index()
        assert np.array_equal(lab, labels) and np.array_equal(c2, cen) and counts.tolist() == SIZES + [N_GIVEN - sum(SIZES)]
        qids = np.random.default_rng(D).permutation(N_GIVEN)[:300].astype(np.uint32)
        vec = clustered(33, D, 9, D + 2)
        S, SC = R.scores(X[qids], X, metric), R.scores(X[qids], cen, metric)
        Sv, SCv = R.scores(vec, X, metric), R.scores(vec, cen, metric)
        padded = False
        for nprobe in (1, 2, 5):
            for k in (1, 10, 128):
                for nq in (1, 33, 300):
                    want = I.index_ref(X, labels, cen, k, metric, nprobe, qids=qids[:nq], rowptr=eng.rowptr, colids=eng.colids, exclude_self=True, S=S[:nq], SC=SC[:nq])
                    got = eng.index_search(ids=qids[:nq], k=k, metric=metric, nprobe=nprobe, details=True)
                    assert equal(got, want), (nprobe, k, nq)
                    assert np.array_equal(got[2], want[2]) and got[3]["candidates"] == want[3] and got[3]["nprobe"] == nprobe
                    padded |= bool((got[0] == PAD).any()) and nprobe == 1 and k == 128
                want = I.index_ref(X, labels, cen, k, metric, nprobe, vectors=vec, S=Sv, SC=SCv)
                got = eng.index_search(vectors=vec, k=k, metric=metric, nprobe=nprobe, details=True)
                assert equal(got, want) and np.array_equal(got[2], want[2]) and got[3]["candidates"] == want[3], (nprobe, k, "vectors")
        assert padded  # k = 128 with one probe of a short list leaves slots past the last candidate
    finally:
        eng.close()


@gpu
def test_order_rules():
    n, D = 400, 8
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, D)).astype(np.float32)
    X[7] = X[300] = X[150]                       # duplicate rows placed in different lists: ties go to the lower id
    X[20, 0], X[21, 1], X[22, 2] = np.inf, np.nan, -0.0
    X[23] = 0.0                                  # a zero row: cosine's r = 0, and -0 / +0 are one score
    X[24] = -0.0
    labels = (np.arange(n) % 5).astype(np.uint32)  # lists 0..4 hold vertices, 5 and 6 are empty, 7 has a NaN centroid
    labels[labels == 4] = 7
    labels[7], labels[150], labels[300] = 0, 1, 2
    cen = rng.standard_normal((8, D)).astype(np.float32)
    cen[3] = cen[1]                              # two identical centroids: the lower list is probed first
    cen[7, 2] = np.nan                           # a NaN centroid is ranked last
    q_empty = rng.standard_normal(D).astype(np.float32)
    cen[5], cen[6] = 50 * q_empty, 40 * q_empty  # by dot product the query q_empty probes the two empty lists first
    eng = engine_for(X)
    try:
        eng.build_index(labels=labels, centroids=cen)
        qids = np.array([150, 7, 300, 20, 21, 22, 23, 24, 0, 1, 2, 3], dtype=np.uint32)
        for metric in METRICS:
            for nprobe in (1, 3, 7, 8):
                for flags in ((False, False), (True, False)):
                    want = I.index_ref(X, labels, cen, 20, metric, nprobe, qids=qids, rowptr=eng.rowptr, colids=eng.colids, exclude_self=flags[0])
                    got = eng.index_search(ids=qids, k=20, metric=metric, nprobe=nprobe, exclude_self=flags[0], details=True)
                    assert equal(got, want) and np.array_equal(got[2], want[2]) and got[3]["candidates"] == want[3], (metric, nprobe, flags)
                    plain = got[2][[0, 8, 9, 10, 11]].tolist()  # the queries without inf / NaN / all-zero rows: every centroid but 7 scores a number
                    if nprobe == 8:
                        assert all(row[7] == 7 and row.index(3) == row.index(1) + 1 for row in plain), plain
                    else:
                        assert not any(7 in row for row in plain), plain
        # the duplicates: all three lists probed, no exclusion -- 7, 150, 300 lead in that order with one score
        ids, sc = eng.index_search(ids=[150], k=3, metric="l2", nprobe=8, exclude_self=False)
        assert ids[0].tolist() == [7, 150, 300] and np.all(sc[0] == 0)
        # a query whose probed lists are all empty: pure padding, no candidates
        ids, sc, pr, info = eng.index_search(vectors=q_empty[None], k=5, metric="dot", nprobe=2, details=True)
        assert pr[0].tolist() == [5, 6] and np.all(ids == PAD) and np.all(sc == -np.inf) and info["candidates"] == 0
    finally:
        eng.close()


@gpu
def test_kmeans_form_is_the_clustering_call():
    X = clustered(2000, 40, 20, 4)
    eng = engine_for(X)
    try:
        for lists, iters, seed in ((25, 6, 3), (1, 3, 1), (130, 2, 9)):
            info = eng.build_index(lists=lists, max_iters=iters, seed=seed)
            km = eng.kmeans(lists, max_iters=iters, seed=seed, restarts=1)
            labels, cen, counts = eng.index()
            assert np.array_equal(labels, km.labels) and np.array_equal(cen.view(np.uint32), km.centroids.view(np.uint32))
            assert np.array_equal(counts, km.counts)
            assert (info.lists, info.inertia, info.iterations, info.converged) == (lists, km.inertia, km.iterations, km.converged)
            assert info.largest == int(counts.max()) and info.empty == int((counts == 0).sum())
            assert info.bytes == 4 * (2 * 2000 + lists + 1) + 4 * lists * 40
        init = X[::100][:20].copy()
        info = eng.build_index(lists=20, max_iters=4, init=init)
        km = eng.kmeans(20, max_iters=4, init=init)
        labels, cen, _ = eng.index()
        assert np.array_equal(labels, km.labels) and np.array_equal(cen.view(np.uint32), km.centroids.view(np.uint32))
        assert (info.inertia, info.iterations, info.converged) == (km.inertia, km.iterations, km.converged)
        assert eng.build_index().lists == 45  # round(sqrt(2000))
    finally:
        eng.close()


@gpu
def test_results_do_not_depend_on_grouping_tunables_handle_or_other_calls():
    D = 40
    X = clustered(N_GIVEN, D, 9, 31)
    labels, cen = given_partition(N_GIVEN, D, 32)
    qids = np.random.default_rng(33).permutation(N_GIVEN)[:300].astype(np.uint32)
    vec = clustered(70, D, 9, 34)

    def search(eng):
        out = []
        for metric in METRICS:
            out += list(eng.index_search(ids=qids, k=10, metric=metric, nprobe=3, details=True)[:3])
            out += list(eng.index_search(vectors=vec, k=10, metric=metric, nprobe=3, details=True)[:3])
        return out

    def same(a, b):
        return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

    eng = engine_for(X)
    try:
        eng.build_index(labels=labels, centroids=cen)
        base = search(eng)
        for metric in METRICS:  # one query per call
            want = eng.index_search(ids=qids, k=10, metric=metric, nprobe=3, details=True)
            for i in range(0, 300, 7):
                got = eng.index_search(ids=qids[i:i + 1], k=10, metric=metric, nprobe=3, details=True)
                assert all(np.array_equal(g[0], w[i]) for g, w in zip(got[:3], want[:3])), (metric, i)
        for name, value, back in (("index_chunk", 64, 8192), ("index_chunk", 1, 8192), ("index_split_tiles", 1, 8), ("index_split_tiles", 3, 8), ("index_block", 32, 0),
                                  ("nearest_chunk", 64, 8192), ("nearest_splits", 3, 0), ("nearest_block", 32, 0), ("nearest_block", 128, 0)):
            eng.set_param(name, value)
            assert eng.get_param(name) == value
            assert same(search(eng), base), (name, value)
            eng.set_param(name, back)
        # the index survives the other scorers' workspaces
        lab7 = np.arange(N_GIVEN) % 7
        eng.nearest(k=100, metric="cos")
        eng.kmeans(300, max_iters=3, seed=5)
        eng.silhouette(lab7)
        eng.pca(2)
        eng.neighbour_recall(10, "l2")
        assert same(search(eng), base)
        lab, c2, _ = eng.index()
        assert np.array_equal(lab, labels) and np.array_equal(c2, cen)
    finally:
        eng.close()
    fresh = engine_for(X)
    try:
        fresh.build_index(labels=labels, centroids=cen)
        assert same(search(fresh), base)
    finally:
        fresh.close()


@gpu
def test_the_index_holds_no_copy_of_the_matrix():
    D = 40
    X, X2 = clustered(N_GIVEN, D, 9, 41), clustered(N_GIVEN, D, 9, 42)
    eng = engine_for(X)
    try:
        eng.build_index(lists=12, max_iters=5, seed=2)
        labels, cen, _ = eng.index()
        eng.set_embeddings(X2)
        lab2, cen2, _ = eng.index()
        assert np.array_equal(lab2, labels) and np.array_equal(cen2, cen)  # the partition is the old one ...
        qids = np.arange(0, N_GIVEN, 5, dtype=np.uint32)
        for metric in METRICS:  # ... the scores and the queries' vectors are the new matrix's
            want = eng.nearest(ids=qids, k=10, metric=metric)
            got = eng.index_search(ids=qids, k=10, metric=metric, nprobe=12)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            want = I.index_ref(X2, labels, cen, 10, metric, 2, qids=qids, rowptr=eng.rowptr, colids=eng.colids, exclude_self=True)
            got = eng.index_search(ids=qids, k=10, metric=metric, nprobe=2, details=True)
            assert equal(got, want) and np.array_equal(got[2], want[2]) and got[3]["candidates"] == want[3]
        # a rebuild replaces the partition
        given, gc = given_partition(N_GIVEN, D, 43)
        eng.build_index(labels=given, centroids=gc)
        lab3, cen3, counts = eng.index()
        assert np.array_equal(lab3, given) and np.array_equal(cen3, gc) and len(counts) == 10
        want = I.index_ref(X2, given, gc, 10, "l2", 2, qids=qids, rowptr=eng.rowptr, colids=eng.colids, exclude_self=True)
        assert equal(eng.index_search(ids=qids, k=10, metric="l2", nprobe=2), want)
        eng.drop_index()
        eng.drop_index()  # nothing to drop: fine
        with pytest.raises(F.F2VError) as e:
            eng.index_search(ids=qids, k=10, nprobe=2)
        assert e.value.code == _lib.F2V_ESTATE and "no index" in str(e.value)
        with pytest.raises(F.F2VError) as e:
            eng.index()
        assert e.value.code == _lib.F2V_ESTATE
    finally:
        eng.close()


@gpu
def test_an_index_changes_neither_training_nor_the_other_queries():
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))

    def run(with_index):
        eng = F.Engine(rowptr, colids, 128)
        try:
            eng.srand(1)
            eng.init_embeddings(0)
            eng.train(5, 5, 256, 5, 0.02)
            if with_index:
                eng.build_index(lists=30, max_iters=5)
                for metric in METRICS:
                    eng.index_search(ids=np.arange(300), k=10, metric=metric, nprobe=4, exclude_neighbours=True)
                eng.index_search(vectors=np.ones((3, 128), dtype=np.float32), k=5, nprobe=2)
            eng.train(5, 5, 256, 5, 0.02)
            X = eng.get_embeddings()
            draw = eng.rand_index(1 << 30)
            km = eng.kmeans(9, max_iters=4, seed=2)
            return X, draw, eng.nearest(ids=np.arange(200), k=10, metric="cos"), eng.neighbour_recall(10, "l2"), km.labels, km.centroids, km.inertia
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1]
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1]) and a[3] == b[3]
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5].view(np.uint32), b[5].view(np.uint32)) and a[6] == b[6]


@gpu
def test_recall_never_falls_as_more_lists_are_probed():
    X = clustered(2000, 16, 32, 51, spread=0.8)  # planted clusters that overlap: one probe does not find everything
    eng = engine_for(X)
    try:
        eng.build_index(lists=32, max_iters=10, seed=1)
        want, _ = eng.nearest(k=10, metric="l2")
        before, first = np.zeros(2000, dtype=np.int64), None
        for nprobe in (1, 2, 4, 8, 16, 32):
            got, _ = eng.index_search(k=10, metric="l2", nprobe=nprobe)
            found = np.array([len(np.intersect1d(g, w)) for g, w in zip(got, want)])
            assert np.all(found >= before), nprobe
            before = found
            first = found.sum() if first is None else first
            assert eng.index_recall(k=10, metric="l2", nprobe=nprobe) == (int(found.sum()), 20000)
        assert np.all(before == 10) and 0 < first < 20000
    finally:
        eng.close()


@gpu
def test_state_and_argument_errors():
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 16)
    try:
        L, h = eng._L, eng._h
        u32, f32 = _lib.u32p, _lib.f32p
        q = np.array([1, 2], dtype=np.uint32)
        oi, os_ = np.zeros((2, 10), dtype=np.uint32), np.zeros((2, 10), dtype=np.float32)
        labels, cen = np.zeros(n, dtype=np.uint32), np.zeros((1100, 16), dtype=np.float32)
        vec = np.ones((2, 16), dtype=np.float32)

        def failed(rc, code, word):
            return rc == code and word in L.f2v_last_error().decode()

        def rows(k=10, metric=0, flags=0, nq=2, nprobe=4, out=oi):
            return L.f2v_index_search_rows(h, q.ctypes.data_as(u32), nq, k, metric, flags, nprobe, out.ctypes.data_as(u32) if out is not None else None,
                                           os_.ctypes.data_as(f32), None, None)

        def vectors(k=10, metric=0, nprobe=4, src=vec):
            return L.f2v_index_search_vectors(h, src.ctypes.data_as(f32) if src is not None else None, 2, k, metric, nprobe, oi.ctypes.data_as(u32), None, None, None)

        def given(lab=labels, c=cen, lists=3):
            return L.f2v_index_build_given(h, lab.ctypes.data_as(u32) if lab is not None else None, c.ctypes.data_as(f32) if c is not None else None, lists, None)

        # no index, no embeddings
        assert failed(rows(), _lib.F2V_ESTATE, "no index") and failed(vectors(), _lib.F2V_ESTATE, "no index")
        assert failed(L.f2v_index_get(h, None, None, None, None), _lib.F2V_ESTATE, "no index")
        assert failed(L.f2v_index_build(h, 4, 5, 1, None, None), _lib.F2V_ESTATE, "never initialised")
        # the given form needs no embeddings; a search does
        assert given() == _lib.F2V_OK
        assert failed(rows(), _lib.F2V_ESTATE, "never initialised")
        eng.set_embeddings(clustered(n, 16, 5, 61))
        for lists in (0, n + 1, 1025):
            assert failed(L.f2v_index_build(h, lists, 5, 1, None, None), _lib.F2V_EINVAL, "lists") and failed(given(lists=lists), _lib.F2V_EINVAL, "lists")
        assert failed(given(lab=None), _lib.F2V_EINVAL, "null") and failed(given(c=None), _lib.F2V_EINVAL, "null")
        labels[n - 1] = 3
        assert failed(given(), _lib.F2V_EINVAL, "not a list")
        labels[n - 1] = 2
        assert rows() == _lib.F2V_OK  # a refused build leaves the index as it was
        assert given() == _lib.F2V_OK
        assert failed(rows(nprobe=0), _lib.F2V_EINVAL, "nprobe") and failed(rows(nprobe=129), _lib.F2V_EINVAL, "nprobe")
        assert failed(vectors(nprobe=0), _lib.F2V_EINVAL, "nprobe") and failed(vectors(nprobe=129), _lib.F2V_EINVAL, "nprobe")
        assert failed(rows(k=0), _lib.F2V_EINVAL, "k = 0") and failed(rows(k=129), _lib.F2V_EINVAL, "k = 129") and failed(vectors(k=0), _lib.F2V_EINVAL, "k = 0")
        assert failed(rows(metric=3), _lib.F2V_EINVAL, "metric") and failed(vectors(metric=-1), _lib.F2V_EINVAL, "metric")
        assert failed(rows(flags=4), _lib.F2V_EINVAL, "flag")
        assert failed(rows(out=None), _lib.F2V_EINVAL, "null") and failed(vectors(src=None), _lib.F2V_EINVAL, "null")
        q[1] = n
        assert failed(rows(), _lib.F2V_EINVAL, "not a vertex")
        q[1] = 2
        oi[:] = 12345
        assert rows(nq=0) == _lib.F2V_OK and np.all(oi == 12345)  # no queries: nothing touched
        assert rows() == _lib.F2V_OK and np.all(oi < n)
        assert rows(nprobe=128) == _lib.F2V_OK and vectors(nprobe=128) == _lib.F2V_OK  # clipped to the 3 lists
    finally:
        eng.close()
    small = engine_for(clustered(34, 8, 3, 62))  # karate: fewer vertices than F2V_INDEX_MAX_LISTS
    try:
        assert small._L.f2v_index_build(small._h, 35, 5, 1, None, None) == _lib.F2V_EINVAL and "lists = 35" in small._L.f2v_last_error().decode()
        assert small.build_index(lists=34, max_iters=2).lists == 34
    finally:
        small.close()
    shuffled = colids.copy()
    lo, hi = rowptr[1], rowptr[2]
    shuffled[lo:hi] = shuffled[lo:hi][::-1]
    if hi - lo > 1:  # a row descending: a row search would miss neighbours
        eng = F.Engine(rowptr, shuffled, 16)
        try:
            eng.set_embeddings(clustered(n, 16, 5, 61))
            eng.build_index(lists=4, max_iters=2)
            eng.index_search(ids=[0, 1], k=5, nprobe=2)
            with pytest.raises(F.F2VError) as e:
                eng.index_search(ids=[0, 1], k=5, nprobe=2, exclude_neighbours=True)
            assert e.value.code == _lib.F2V_EINVAL and "ascending" in str(e.value)
        finally:
            eng.close()


@gpu
def test_cli_sweeps_through_the_index(tmp_path):
    mtx = golden_graph_path("cora.mtx")
    outs = {}
    for name, extra in (("exact", []), ("all", ["-nearest-lists", "16", "-nearest-probes", "16"]),
                        ("some", ["-nearest-lists", "16", "-nearest-probes", "2", "-nearest-check", "100"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([CLI, "-input", mtx, "-iter", "30", "-batch", "256", "-output", str(d) + "/", "-nearest", "5"] + extra,
                           capture_output=True, text=True, cwd=d, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        nn = [p for p in os.listdir(d) if p.endswith(".nn")]
        assert len(nn) == 1
        outs[name] = (r.stdout, open(d / nn[0], "rb").read())
    assert outs["exact"][1] == outs["all"][1] and "Index:" not in outs["exact"][0]
    precision = lambda text: re.search(r"precision@k (\d+)/(\d+)", text).groups()
    assert precision(outs["exact"][0]) == precision(outs["all"][0])
    m = re.search(r"Index: lists 16 probes 16 candidates/query (\S+)", outs["all"][0])
    assert m and float(m.group(1)) == 2708.0
    m = re.search(r"Index: lists 16 probes 2 candidates/query (\S+)", outs["some"][0])
    assert m and 0 < float(m.group(1)) < 2708.0
    m = re.search(r"Recall@5 against the exact search \(100 vertices\): (\S+)", outs["some"][0])
    assert m and 0 < float(m.group(1)) <= 1
    assert len(outs["some"][1].splitlines()) == 2708
