"""Held-out link prediction (include/f2v.h: f2v_edge_split, f2v_pair_scores, f2v_ranking; Engine.edge_split / pair_scores / ranking /
heldout_scores; bin/Force2Vec -holdout).

Host tests: the restatement tests/heldout_ref.py against the properties the definitions promise -- the split conserves the nonzeros,
is symmetric, leaves every vertex a neighbour; the ranking's tallies equal a count over all (one, zero) pairs and its two measures
equal scikit-learn's within 1e-11 (m <= 10^4 fp64 roundings of 1.1e-16, tenfold margin).  -m gpu: the three calls bit for bit against
the restatement, the calling convention, one end-to-end run on cora against the CPU oracle, and the command-line flag."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import heldout_ref as R
from test_gather_isa import FLAGS, HIPCC, function
from test_linkpairs import both, csr
from test_logreg import spills

gpu = pytest.mark.gpu
CLI = os.path.join(ROOT, "bin", "Force2Vec")
ARRAYS = ("rowptr", "colids", "held_u", "held_v", "neg_u", "neg_v")
# (frac, ratio) of the issue
COMBOS = ((0.0, 1), (0.3, 1), (0.999, 1), (0.5, 1), (0.5, 16))


def mixed():
    """a duplicated nonzero and a self-loop (row 7), an isolated vertex (5), a nonzero stored in one direction only (20 -> 250)"""
    n, rng = 300, np.random.default_rng(11)
    plain = np.array([v for v in range(n) if v != 5])
    und = {(int(min(a, b)), int(max(a, b))) for a, b in zip(rng.choice(plain, 3 * n), rng.choice(plain, 3 * n)) if a != b}
    und |= {(7, 200), (20, 21)}
    und.discard((20, 250))
    return csr(n, both(sorted(und)) + [(7, 7), (7, 200), (20, 250)])


def hub():
    """n = 8192: vertex 0 has 1000 neighbours, vertex 2000 has 100; every neighbour is also tied to the next three, so that the hub's
    edge is seldom the one its anchor rule protects"""
    und = {(0, v) for v in range(1, 1001)} | {(v, v + d) for v in range(1, 1001) for d in (1, 2, 3) if v + d <= 1000}
    und |= {(2000, v) for v in range(2001, 2101)} | {(v, v + d) for v in range(2001, 2101) for d in (1, 2, 3) if v + d <= 2100}
    return csr(8192, both(sorted(und)))


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in ("karate", "cora"):
        return F.read_mtx(golden_graph_path(name + ".mtx"))
    return {"mixed": mixed, "hub": hub}[name]()


@functools.lru_cache(maxsize=None)
def restated(name, frac, ratio, seed=1):
    """shared, never modified"""
    return R.split(*graph(name), frac, seed=seed, ratio=ratio)


def nonzeros(rowptr, colids):
    return [(u, int(v)) for u in range(len(rowptr) - 1) for v in colids[rowptr[u]:rowptr[u + 1]]]


# ---- host: the split restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karate", "mixed", "hub"])
def test_frac_zero_holds_nothing(name):
    rowptr, colids = graph(name)
    s = restated(name, 0.0, 1)
    assert np.array_equal(s["rowptr"], rowptr) and np.array_equal(s["colids"], colids)
    assert s["held"] == s["negatives"] == s["candidates_held"] == s["protected"] == 0 and len(s["held_u"]) == len(s["neg_u"]) == 0


@pytest.mark.parametrize("name,frac", [("karate", 0.3), ("karate", 0.999), ("cora", 0.3), ("hub", 0.5), ("mixed", 0.5)])
def test_split_conserves_the_nonzeros_and_keeps_every_vertex_a_neighbour(name, frac):
    rowptr, colids = graph(name)
    s = restated(name, frac, 1)
    n = len(rowptr) - 1
    full, train = nonzeros(rowptr, colids), nonzeros(s["rowptr"], s["colids"])
    held = set(zip(s["held_u"].tolist(), s["held_v"].tolist()))
    assert all(u < v for u, v in held) and len(held) == s["held"] == s["candidates_held"] - s["protected"] > 0
    assert s["train_nnz"] == len(train)
    gone = set(full) - set(train)  # the rule per nonzero: what left the rows are the nonzeros of held pairs, and all of them
    assert {(min(u, v), max(u, v)) for u, v in gone} == held and not any((u, v) in held or (v, u) in held for u, v in train)
    if name == "mixed":
        assert (7, 7) in train and train.count((7, 200)) in (0, 2)  # the self-loop stays; the duplicates go or stay together
    if name in ("karate", "hub"):  # symmetric, no duplicates: the training nonzeros plus the held pairs in both directions are the input nonzeros
        assert sorted(train + [(u, v) for u, v in held] + [(v, u) for u, v in held]) == sorted(full)
    if name != "mixed":  # every nonzero has its mirror: the held set is symmetric
        assert set(train) == {(v, u) for u, v in train}
    for u in range(n):  # order kept inside a row
        row = [v for v in colids[rowptr[u]:rowptr[u + 1]]]
        kept = [v for v in s["colids"][s["rowptr"][u]:s["rowptr"][u + 1]]]
        it = iter(row)
        assert all(v in it for v in kept)
        if any(v != u for v in row):
            assert any(v != u for v in kept), u  # every vertex with a neighbour keeps one
    edges = set(full)
    assert not any((u, v) in edges or (v, u) in edges or u == v for u, v in zip(s["neg_u"].tolist(), s["neg_v"].tolist()))  # non-edges of the FULL graph
    assert len(set(zip(s["neg_u"].tolist(), s["neg_v"].tolist()))) == s["negatives"] == sum(s["total"])


def test_the_anchors_lower_the_held_share_below_frac():
    """A candidate is an edge of SMALL key and a vertex's anchor is its edge of smallest key: every vertex that has a candidate at all
    protects one.  So protected <= the vertices with a neighbour, and on a graph of low degree (cora: 3.9 a vertex) the held share
    falls far below frac.  The candidates themselves are a binomial share of the edges: frac within five standard deviations."""
    rowptr, colids = graph("cora")
    s = restated("cora", 0.3, 1)
    print("cora frac 0.3: edges %d candidates %d protected %d held %d: share %.4f" % (s["edges"], s["candidates_held"], s["protected"], s["held"], s["held"] / s["edges"]))
    assert abs(s["candidates_held"] - 0.3 * s["edges"]) < 5 * (s["edges"] * 0.3 * 0.7) ** 0.5
    assert 0 < s["protected"] <= len(rowptr) - 1 and 0 < s["held"] == s["candidates_held"] - s["protected"]


def test_hub_runs_both_table_forms_and_hits_the_cap():
    s = restated("hub", 0.5, 16)
    assert s["total"][0] > 3072 and s["total"][0] > 1024  # above the largest "link_short_max" too: a table in the workspace
    assert 256 < s["total"][2000] <= 3072                 # above the default "link_short_max": a table in LDS
    assert s["capped"] >= 1 and s["total"][0] == (8192 - 1 - 1000) // 2


# ---- host: the ranking restatement -----------------------------------------------------------------------------------------------
def tied_scores(rng, m):
    s = rng.integers(-3, 4, m).astype(np.float64) / 2.0  # heavy ties
    s[rng.random(m) < 0.1] = -0.0
    s[rng.random(m) < 0.1] = 0.0
    s[rng.random(m) < 0.05] = np.inf
    s[rng.random(m) < 0.05] = -np.inf
    s[rng.random(m) < 0.1] = np.nan
    return s


@pytest.mark.parametrize("m", [2, 17, 300])
def test_restated_tallies_equal_a_count_over_all_pairs(m):
    rng = np.random.default_rng(m)
    for _ in range(5):
        s = tied_scores(rng, m)
        y = (rng.random(m) < 0.4).astype(np.uint8)
        y[0], y[1] = 1, 0
        r = R.ranking(s, y)
        assert (r["concordant"], r["tied"]) == R.pair_count(s, y)
        assert r["concordant"] + r["tied"] <= r["positives"] * r["negatives"] and 0.0 <= r["auc"] <= 1.0 and 0.0 < r["ap"] <= 1.0
        assert r["groups"] == len({R.order_key(x) for x in s})


def test_order_key_orders_as_the_definition_says():
    seq = [np.nan, -np.inf, -1.5, -5e-324, 0.0, 5e-324, 1.0, np.inf]
    keys = [R.order_key(x) for x in seq]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert R.order_key(-0.0) == R.order_key(0.0) and R.order_key(float("nan")) == R.order_key(-float("nan")) == 0


@pytest.mark.parametrize("m", [2, 100, 10000])
def test_restated_measures_equal_scikit_learn(m):
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(m + 1)
    for ties in (False, True):
        s = rng.standard_normal(m)
        if ties:
            s = np.round(s * 4) / 4
        y = (rng.random(m) < 0.3).astype(np.uint8)
        y[0], y[1] = 1, 0
        r = R.ranking(s, y)
        assert abs(r["auc"] - metrics.roc_auc_score(y, s)) <= 1e-11
        assert abs(r["ap"] - metrics.average_precision_score(y, s)) <= 1e-11


def test_entry_points_are_declared():
    for name in ("f2v_edge_split", "f2v_pair_scores", "f2v_ranking"):
        assert name in _lib.SIGNATURES
    for name in ("edge_split", "pair_scores", "ranking", "heldout_scores"):
        assert callable(getattr(F.Engine, name))


def test_cli_help_and_refusals(tmp_path):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-holdout " in r.stdout and "-holdout-ratio" in r.stdout and "-holdout-metric" in r.stdout and "TRAINING GRAPH'S EMBEDDING" in r.stdout
    mtx = golden_graph_path("karate.mtx")
    for extra, word in ((["-gpus", "2"], "-gpus"), (["-foldin", "x"], "-foldin"), (["-holdout-ratio", "17"], "-holdout-ratio"), (["-holdout-metric", "x"], "-holdout-metric")):
        r = subprocess.run([CLI, "-input", mtx, "-holdout", "0.3"] + extra, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and word in r.stdout, (extra, r.stdout)
    for bad in ("1", "-0.5", "1.5"):
        r = subprocess.run([CLI, "-input", mtx, "-holdout", bad], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "-holdout must be" in r.stdout, (bad, r.stdout)
    r = subprocess.run([CLI, "-input", mtx, "-option", "3", "-holdout", "0.3"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "out of scope" in r.stdout


KERNELS = ["held_anchor_kernel", "held_count_kernel", "held_fill_kernel", "pair_score_kernelILi0EE", "pair_score_kernelILi1EE", "pair_score_kernelILi2EE",
           "rank_key_kernel", "rank_scan_tile_kernel", "rank_scan_apply_kernel", "rank_group_kernel", "rank_block_kernel", "rank_total_kernel"]
TU = '#include "f2v_heldout.hip.h"\n' + "".join("template __global__ void f2v::pair_score_kernel<%d>(const f2v::PairArgs);\n" % k for k in range(3))


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "heldout_isa.hip"), str(tmp_path / "heldout_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


# ---- GPU: the split ------------------------------------------------------------------------------------------------------------------
def same_split(got, want):
    return all(np.array_equal(getattr(got, k), want[k]) and getattr(got, k).dtype == np.uint32 for k in ARRAYS) and \
        all(getattr(got.info, k) == want[k] for k in R.SPLIT_COUNTERS)


@gpu
@pytest.mark.parametrize("name", ["karate", "cora", "mixed", "hub"])
def test_split_equals_the_restatement(name):
    eng = F.Engine(*graph(name), 4)
    try:
        for frac, ratio in COMBOS:
            got, want = eng.edge_split(frac=frac, seed=1, ratio=ratio, details=True), restated(name, frac, ratio)
            assert same_split(got, want), (name, frac, ratio, got.info, {k: want[k] for k in R.SPLIT_COUNTERS})
        got = eng.edge_split(frac=0.3, seed=0xC0FFEE123456789, ratio=0, details=True)
        assert same_split(got, restated(name, 0.3, 0, 0xC0FFEE123456789)) and len(got.neg_u) == 0
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name", ["hub", "cora"])
def test_link_short_max_does_not_change_the_split(name):
    want = restated(name, 0.5, 16)
    eng = F.Engine(*graph(name), 4)
    try:
        for value in (0, 1024, 64, 256):
            eng.set_param("link_short_max", value)
            assert same_split(eng.edge_split(frac=0.5, ratio=16, details=True), want), value
    finally:
        eng.close()


def raw_split(eng, frac, seed, ratio, arrays, caps, counts=True):
    ptr = lambda a: a.ctypes.data_as(_lib.u32p) if a is not None else None
    c, info = [C.c_uint64(0xDEAD) for _ in range(3)], _lib.SplitInfo()
    refs = [C.byref(x) if counts else None for x in c]
    rc = eng._L.f2v_edge_split(eng._h, frac, seed, ratio, ptr(arrays[0]), ptr(arrays[1]), caps[0], ptr(arrays[2]), ptr(arrays[3]), caps[1], ptr(arrays[4]),
                               ptr(arrays[5]), caps[2], *refs, C.byref(info))
    return rc, tuple(x.value for x in c), info


@gpu
def test_split_calling_convention_and_refusals():
    want = restated("karate", 0.3, 1)
    sizes = (want["train_nnz"], want["held"], want["negatives"])
    rowptr, colids = graph("karate")
    eng = F.Engine(rowptr, colids, 4)
    message = lambda: eng._L.f2v_last_error().decode()
    none = [None] * 6
    try:
        rc, counts, info = raw_split(eng, 0.3, 1, 1, none, (0, 0, 0))  # count only; the handle has no embeddings
        assert rc == 0 and counts == sizes and info.drawn == 0 and info.held == want["held"] and info.capped == want["capped"]
        fresh = lambda pad=3: [np.full(len(rowptr), 77, dtype=np.uint32)] + [np.full(s + pad, 77, dtype=np.uint32) for s in (sizes[0], sizes[1], sizes[1], sizes[2], sizes[2])]
        arrays = fresh()
        rc, counts, info = raw_split(eng, 0.3, 1, 1, arrays, tuple(s + 3 for s in sizes))
        assert rc == 0 and counts == sizes and info.drawn == want["drawn"] and info.seconds > 0
        for a, k, s in zip(arrays, ARRAYS, (len(rowptr),) + (sizes[0], sizes[1], sizes[1], sizes[2], sizes[2])):
            assert np.array_equal(a[:s], want[k]) and (a[s:] == 77).all(), k
        for short in range(3):  # a capacity too small: F2V_EINVAL with the counts written, nothing else
            arrays = fresh(0)
            caps = tuple(s - (i == short) for i, s in enumerate(sizes))
            rc, counts, _ = raw_split(eng, 0.3, 1, 1, arrays, caps)
            assert rc == _lib.F2V_EINVAL and counts == sizes and all((a == 77).all() for a in arrays) and "arrays hold" in message()
        for frac in (-0.1, 1.0, 1.5, float("nan")):
            assert raw_split(eng, frac, 1, 1, none, (0, 0, 0))[0] == _lib.F2V_EINVAL and "frac" in message()
        assert raw_split(eng, 0.3, 1, 17, none, (0, 0, 0))[0] == _lib.F2V_EINVAL and "ratio" in message()
        arrays = fresh()
        for k in (0, 3, 5):
            partial = list(arrays)
            partial[k] = None
            assert raw_split(eng, 0.3, 1, 1, partial, tuple(s + 3 for s in sizes))[0] == _lib.F2V_EINVAL and "together" in message()
        assert raw_split(eng, 0.3, 1, 1, none, (0, 0, 0), counts=False)[0] == _lib.F2V_EINVAL
    finally:
        eng.close()
    shuffled = colids.copy()
    shuffled[rowptr[0]:rowptr[1]] = shuffled[rowptr[0]:rowptr[1]][::-1]
    eng = F.Engine(rowptr, shuffled, 4)
    try:
        with pytest.raises(F.F2VError, match="f2v_edge_split: the CSR's column ids are not ascending"):
            eng.edge_split()
    finally:
        eng.close()


@gpu
def test_the_calls_touch_neither_the_matrix_nor_the_rand_stream():
    rowptr, colids = graph("karate")
    a, b = F.Engine(rowptr, colids, 16), F.Engine(rowptr, colids, 16)
    try:
        for e in (a, b):
            e.srand(5)
            e.init_embeddings(0)
            e.train(5, 2, 16, 5, 0.02)
        s = a.edge_split(frac=0.3)
        a.heldout_scores(s, metric="cos")
        assert np.array_equal(a.get_embeddings(), b.get_embeddings())
        assert [a.rand_index(1000) for _ in range(8)] == [b.rand_index(1000) for _ in range(8)]
        a.train(5, 2, 16, 5, 0.02)
        b.train(5, 2, 16, 5, 0.02)
        assert np.array_equal(a.get_embeddings(), b.get_embeddings())
    finally:
        a.close()
        b.close()


# ---- GPU: pair scores ----------------------------------------------------------------------------------------------------------------
N_ROWS = 97
M_SIZES = (1, 63, 64, 65, 300)


def matrix(D):
    rng = np.random.default_rng(D)
    X = rng.standard_normal((N_ROWS, D)).astype(np.float32)
    X[3] = 0.0             # a zero row: r_v = 0 under cosine
    X[5, D // 2] = np.inf  # a row with inf
    X[8, 0] = np.nan       # a row with NaN
    return X


def pairs(m):
    rng = np.random.default_rng(m)
    u, v = rng.integers(0, N_ROWS, m).astype(np.uint32), rng.integers(0, N_ROWS, m).astype(np.uint32)
    special = [(4, 4), (3, 7), (7, 3), (3, 3), (5, 9), (9, 5), (8, 2), (2, 8), (5, 8), (12, 13), (12, 13)]  # u == v, the special rows, a repeated pair
    for i, (a, b) in enumerate(special[:m]):
        u[-1 - i], v[-1 - i] = a, b
    return u, v


@gpu
@pytest.mark.parametrize("D", [1, 3, 16, 100, 128, 200])
def test_pair_scores_equal_the_restatement_and_nearest(D):
    X = matrix(D)
    eng = F.Engine(*csr(N_ROWS, []), D)
    try:
        eng.set_embeddings(X)
        for metric in ("dot", "l2", "cos"):
            ids, sc = eng.nearest(k=N_ROWS, metric=metric, exclude_self=False)  # every (query, id) score of the matrix
            table = np.empty((N_ROWS, N_ROWS), dtype=np.float32)
            np.put_along_axis(table, ids.astype(np.int64), sc, axis=1)
            for m in M_SIZES:
                u, v = pairs(m)
                want = R.pair_scores(X, u, v, metric)
                eng.set_param("pairs_chunk", 1 << 20)
                one = eng.pair_scores(u, v, metric)
                eng.set_param("pairs_chunk", 128)  # a call of 300 pairs spans three chunks
                got = eng.pair_scores(u, v, metric)
                assert got.dtype == np.float32 and got.tobytes() == one.tobytes(), (D, metric, m)
                assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want) & ~np.isnan(want)), (D, metric, m)
                assert np.array_equal(got, table[u.astype(np.int64), v.astype(np.int64)], equal_nan=True), (D, metric, m)
    finally:
        eng.close()


@gpu
def test_pair_scores_refusals():
    bare = F.Engine(*csr(N_ROWS, []), 8)
    try:
        with pytest.raises(F.F2VError) as e:
            bare.pair_scores([1], [2])
        assert e.value.code == _lib.F2V_ESTATE
        bare.set_embeddings(matrix(8))
        assert len(bare.pair_scores([], [])) == 0
        for u, v, metric in (([N_ROWS], [0], "dot"), ([0], [N_ROWS], "dot"), ([0], [1], 7)):
            with pytest.raises(F.F2VError) as e:
                bare.pair_scores(u, v, metric)
            assert e.value.code == _lib.F2V_EINVAL
        assert bare._L.f2v_pair_scores(bare._h, None, None, 3, 0, None, None) == _lib.F2V_EINVAL
    finally:
        bare.close()


# ---- GPU: ranking ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranker():
    eng = F.Engine(*graph("karate"), 4)
    yield eng
    eng.close()


def same_ranking(got, want):
    return all(getattr(got, k) == want[k] for k in ("concordant", "tied", "positives", "negatives", "groups")) and \
        np.float64(got.auc).tobytes() == np.float64(want["auc"]).tobytes() and np.float64(got.ap).tobytes() == np.float64(want["ap"]).tobytes()


@gpu
@pytest.mark.parametrize("m", [2, 1023, 1024, 1025, 5000])
def test_ranking_equals_the_restatement_under_every_order(ranker, m):
    rng = np.random.default_rng(m)
    for kind in ("ties", "plain"):
        s = tied_scores(rng, m) if kind == "ties" else rng.standard_normal(m).astype(np.float32).astype(np.float64)
        y = (rng.random(m) < 0.4).astype(np.uint8)
        y[0], y[1] = 1, 0
        want = R.ranking(s, y)
        got = ranker.ranking(s, y)
        assert same_ranking(got, want), (m, kind, got, want)
        p = rng.permutation(m)
        assert tuple(ranker.ranking(s[p], y[p]))[:-1] == tuple(got)[:-1], (m, kind)  # a shuffled input: identical bits
    y = (np.arange(m) % 2).astype(np.uint8)
    tied = ranker.ranking(np.full(m, 0.25), y)
    P = float(tied.positives)
    assert tied.auc == 0.5 and tied.groups == 1 and tied.ap == ((P * P) / float(m)) / P  # all scores tied: one group, one term
    sep = ranker.ranking(np.where(y == 1, 2.0, -1.0) + 0.001 * np.arange(m) * (2 * y.astype(np.float64) - 1), y)
    assert sep.auc == 1.0 and sep.ap == 1.0 and sep.tied == 0  # perfectly separated


@gpu
def test_ranking_refusals(ranker):
    for y in ([1, 1, 1], [0, 0], [0, 1, 2]):
        with pytest.raises(F.F2VError) as e:
            ranker.ranking(np.zeros(len(y)), y)
        assert e.value.code == _lib.F2V_EINVAL
    with pytest.raises(F.F2VError):
        ranker.ranking([], [])


# ---- GPU: end to end ---------------------------------------------------------------------------------------------------------------
EPOCHS = 30


@functools.lru_cache(maxsize=None)
def cora_run():
    """cora, frac 0.3, seed 1; option 5, D = 16, batch 256, EPOCHS epochs from srand(1) on the training CSR
    -> (split, the trained matrix, the initial matrix, heldout_scores of both for every metric)"""
    from oracle import oracle as O
    s = restated("cora", 0.3, 1)
    split = F.EdgeSplit(*(s[k] for k in ARRAYS))
    eng = F.Engine(split.rowptr, split.colids, 16)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        X0 = eng.get_embeddings()
        before = {m: eng.heldout_scores(split, metric=m) for m in ("dot", "l2", "cos")}
        eng.train(5, EPOCHS, 256, 5, 0.02)
        X = eng.get_embeddings()
        after = {m: eng.heldout_scores(split, metric=m) for m in ("dot", "l2", "cos")}
        clf = eng.heldout_scores(split, metric="l2", feature="hadamard")
        want = O.train(5, split.rowptr, split.colids, 16, EPOCHS, 256, order=O.ORDER_TREE, chunk=eng.get_param("hub_chunk"))
        return split, X, X0, before, after, clf, want
    finally:
        eng.close()


def restated_scores(X, split, metric):
    u, v = np.concatenate([split.held_u, split.neg_u]), np.concatenate([split.held_v, split.neg_v])
    y = np.concatenate([np.ones(len(split.held_u), dtype=np.uint8), np.zeros(len(split.neg_u), dtype=np.uint8)])
    return R.ranking(R.pair_scores(X, u, v, metric).astype(np.float64), y)


@gpu
def test_cora_end_to_end_against_the_oracle_and_the_restatement():
    split, X, X0, before, after, clf, want = cora_run()
    assert np.array_equal(X, want)  # the engine on the training CSR and the CPU oracle on the same CSR: one matrix
    for metric in ("dot", "l2", "cos"):
        for M, got in ((X, after[metric]), (X0, before[metric])):
            r = restated_scores(M, split, metric)
            assert np.float64(got.auc).tobytes() == np.float64(r["auc"]).tobytes() and np.float64(got.ap).tobytes() == np.float64(r["ap"]).tobytes(), metric
    print("cora held-out (l2): untrained AUC %.6f AP %.6f; after %d epochs AUC %.6f AP %.6f; classifier(hadamard) AUC %.6f AP %.6f"
          % (before["l2"].auc, before["l2"].ap, EPOCHS, after["l2"].auc, after["l2"].ap, clf.classifier_auc, clf.classifier_ap))
    assert after["l2"].auc > before["l2"].auc  # training on the rest predicts the hidden edges better than the initial matrix
    assert (clf.auc, clf.ap) == (after["l2"].auc, after["l2"].ap) and 0.0 < clf.classifier_auc <= 1.0 and 0.0 < clf.classifier_ap <= 1.0


@gpu
def test_cli_holdout_writes_the_pairs_and_prints_the_engines_scores(tmp_path):
    mtx = golden_graph_path("karate.mtx")
    r = subprocess.run([CLI, "-input", mtx, "-iter", "20", "-dim", "16", "-batch", "16", "-option", "5", "-binout", "1", "-seed", "1", "-holdout", "0.3", "-holdout-ratio", "2",
                        "-linkpredict", "hadamard", "-output", str(tmp_path) + "/"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = restated("karate", 0.3, 2)
    held = [p for p in os.listdir(tmp_path) if p.endswith(".held")]
    embd = [p for p in os.listdir(tmp_path) if p.endswith(".embd")]
    assert len(held) == 1 and len(embd) == 1 and held[0] == embd[0] + ".held"
    lines = np.loadtxt(str(tmp_path / held[0]), dtype=np.int64).reshape(-1, 3)
    assert len(lines) == want["held"] + want["negatives"]
    assert np.array_equal(lines[:, 0] - 1, np.concatenate([want["held_u"], want["neg_u"]])) and np.array_equal(lines[:, 1] - 1, np.concatenate([want["held_v"], want["neg_v"]]))
    assert np.array_equal(lines[:, 2], np.concatenate([np.ones(want["held"]), np.zeros(want["negatives"])]))
    split = F.EdgeSplit(*(want[k] for k in ARRAYS))
    eng = F.Engine(split.rowptr, split.colids, 16)
    try:
        eng.set_embeddings(F.read_embd_bin(str(tmp_path / embd[0]) + ".bin", len(split.rowptr) - 1, 16))  # the training graph's embedding
        scores = eng.heldout_scores(split, metric="l2", feature="hadamard", seed=1)
    finally:
        eng.close()
    m = re.search(r"^Held-out link prediction\(l2\): (\d+) edges :AUC: (\S+) AP: (\S+)$", r.stdout, re.M)
    c = re.search(r"^Held-out link prediction\(Hadamard\): (\d+) edges :AUC: (\S+) AP: (\S+)$", r.stdout, re.M)
    assert m and c, r.stdout
    assert int(m.group(1)) == want["held"] and (float(m.group(2)), float(m.group(3))) == (scores.auc, scores.ap)
    assert (float(c.group(2)), float(c.group(3))) == (scores.classifier_auc, scores.classifier_ap)
    r = subprocess.run([CLI, "-input", mtx, "-holdout", "0.3", "-gpus", "2"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-holdout is not available with -gpus" in r.stdout
