"""Components, spanning forests, the connected split and induced subgraphs (include/f2v.h: f2v_components, f2v_spanning_forest,
f2v_edge_split_connected, f2v_subgraph; Engine.components / spanning_forest / edge_split(keep="forest") / subgraph /
largest_component; bin/Force2Vec -components, -holdout-keep).

Host tests: the restatement tests/components_ref.py against a breadth-first search and against the properties the definitions promise
(the least forest holds every anchor edge of the merged split; the connected split keeps the components; it hides at least twice the
edges of the anchor rule on cora).  -m gpu: every call bit for bit against the restatement, the calling conventions, the command line.
Everything is integers and every result is unique by definition, so every comparison is array_equal."""
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
import components_ref as R
import heldout_ref as H
from test_gather_isa import FLAGS, HIPCC, function
from test_linkpairs import both, csr
from test_logreg import spills

gpu = pytest.mark.gpu
CLI = os.path.join(ROOT, "bin", "Force2Vec")
GRAPHS = ("karate", "cora", "pieces")
ARRAYS = ("rowptr", "colids", "held_u", "held_v", "neg_u", "neg_v")
ONE_WAY = range(5200, 5240)  # the vertices of `pieces` whose edges are stored in one direction only


def pieces():
    """n = 6000.  Every id not named below is isolated (0..4, 6..9, 311..399, ...).  5: its only nonzero is a self-loop.  10: a star with the 300
    leaves 11..310 -- a row longer than 256 nonzeros -- with the nonzero (10, 11) stored twice.  400..419 and 420..439: two 20-cliques
    joined by the bridge {419, 420}, the nonzeros of {400, 401} stored twice in both rows.  1000..5095: a path of 4096 consecutive ids.
    5200..5239: a random tree plus a few more edges, every edge stored in ONE direction only, the directions mixed."""
    rng = np.random.default_rng(7)
    und = {(10, v) for v in range(11, 311)}
    for base in (400, 420):
        und |= {(a, b) for a in range(base, base + 20) for b in range(a + 1, base + 20)}
    und |= {(419, 420)}
    und |= {(v, v + 1) for v in range(1000, 5095)}
    nz = both(sorted(und)) + [(5, 5), (10, 11), (400, 401), (401, 400)]
    one = {(int(rng.integers(5200, v)), v) for v in range(5201, 5240)}
    one |= {(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(5200, 5240, (12, 2)) if a != b}
    nz += [(a, b) if i % 2 else (b, a) for i, (a, b) in enumerate(sorted(one))]
    return csr(6000, nz)


@functools.lru_cache(maxsize=None)
def graph(name):
    return pieces() if name == "pieces" else F.read_mtx(golden_graph_path(name + ".mtx"))


@functools.lru_cache(maxsize=None)
def comps(name):
    """shared, never modified"""
    return R.components(*graph(name))


@functools.lru_cache(maxsize=None)
def forest(name, seed, greatest, bits):
    return R.forest(*graph(name), seed, greatest, bits)


@functools.lru_cache(maxsize=None)
def connected(name, frac, ratio, seed=1):
    return R.split_connected(*graph(name), frac, seed, ratio)


def labels_of(rowptr, colids):
    return R.components(rowptr, colids)["labels"]


# ---- host -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_restatement_agrees_with_breadth_first_search(name):
    c = comps(name)
    assert np.array_equal(c["labels"], R.bfs_labels(*graph(name)))
    assert c["components"] == len(set(c["labels"].tolist())) and c["sizes"].sum() == sum(s * s for s in np.bincount(c["labels"]).tolist())
    if name == "karate":
        assert c["components"] == 1 and c["isolated"] == 0 and c["largest"] == 34
    if name == "cora":
        assert (c["components"], c["largest"], c["edges"]) == (78, 2485, 5278)
    if name == "pieces":
        n = 6000
        assert c["isolated"] == n - (301 + 40 + 4096 + 40) and c["sizes"][5] == 1 and c["largest"] == 4096 and c["largest_label"] == 1000
        assert c["components"] == c["isolated"] + 4 and c["labels"][5239] == 5200 and c["sizes"][10] == 301 and c["sizes"][439] == 40


@pytest.mark.parametrize("name", GRAPHS)
def test_forests_span_the_components_and_differ_by_direction(name):
    c = comps(name)
    n = len(c["labels"])
    und = set(R.pairs(*graph(name)))
    for bits in (64, 2, 1):
        got = {}
        for greatest in (False, True):
            u, v = forest(name, 1, greatest, bits)
            assert len(u) == n - c["components"] and (u < v).all() and set(zip(u.tolist(), v.tolist())) <= und
            assert list(zip(u.tolist(), v.tolist())) == sorted(zip(u.tolist(), v.tolist()))
            rp, ci = csr(n, both(list(zip(u.tolist(), v.tolist()))))
            assert np.array_equal(labels_of(rp, ci), c["labels"])  # a spanning forest: the graph's components with the fewest edges
            got[greatest] = set(zip(u.tolist(), v.tolist()))
        if name != "pieces" or bits == 64:
            assert got[False] != got[True]
    if name == "pieces":  # with one or two key bits the order along the path falls back to (a, b): long runs of equal keys
        se, _ = H.seeds(1)
        path = [(v, v + 1) for v in range(1000, 5095)]
        assert len({k >> 63 for k in R.pair_keys(se, path)}) == 2


@pytest.mark.parametrize("name", GRAPHS)
def test_least_forest_contains_every_anchor_edge(name):
    """The link to the merged rule: anchor(u) is u's edge of smallest (key, id), and the smallest edge at a vertex is in the least
    spanning forest (the cut property).  On `pieces` the one-directional vertices are left out: their rows do not show all their edges."""
    rowptr, colids = graph(name)
    se, _ = H.seeds(1)
    u, v = forest(name, 1, False, 64)
    least = set(zip(u.tolist(), v.tolist()))
    anchors = 0
    for x in range(len(rowptr) - 1):
        nb = H.neighbours(rowptr, colids, x)
        if len(nb) == 0 or x in ONE_WAY and name == "pieces":
            continue
        k = H.keys(se, x, nb)
        a = min(zip(k, nb.tolist()))[1]
        assert (min(x, a), max(x, a)) in least, (x, a)
        anchors += 1
    assert anchors > 30


@pytest.mark.parametrize("name,frac", [("karate", 0.3), ("cora", 0.3), ("cora", 0.9), ("pieces", 0.3), ("pieces", 0.9)])
def test_connected_split_keeps_the_components(name, frac):
    s = connected(name, frac, 0)
    assert s["held"] > 0 and s["held"] == s["candidates_held"] - s["protected"]
    assert np.array_equal(labels_of(s["rowptr"], s["colids"]), comps(name)["labels"])
    fu, fv = forest(name, 1, True, 64)
    assert not set(zip(s["held_u"].tolist(), s["held_v"].tolist())) & set(zip(fu.tolist(), fv.tolist()))


def test_forest_split_holds_at_least_twice_the_anchor_split_on_cora():
    """The issue's condition, with the real mix64 keys: cora, frac 0.3, seed 1.  Measured: anchor rule 386 of 5278 edges (7.3 %),
    forest rule 1368 (25.9 %): 3.54 times."""
    anchor, tree = H.split(*graph("cora"), 0.3, seed=1, ratio=0), connected("cora", 0.3, 0)
    print("cora frac 0.3 seed 1: edges %d candidates %d; held by the anchor rule %d, by the forest rule %d: ratio %.3f"
          % (tree["edges"], tree["candidates_held"], anchor["held"], tree["held"], tree["held"] / anchor["held"]))
    assert anchor["candidates_held"] == tree["candidates_held"] and anchor["edges"] == tree["edges"] == 5278
    assert tree["held"] >= 2 * anchor["held"]


def test_subgraph_restatement():
    rowptr, colids = graph("pieces")
    keep = comps("pieces")["labels"] == 400
    rp, ci, ids, new_id = R.subgraph(rowptr, colids, keep)
    assert len(ids) == 40 and rp[-1] == 2 * (2 * 190 + 1) + 2 and np.array_equal(ids, np.arange(400, 440))
    assert (new_id[~keep] == R.DROPPED).all() and np.array_equal(new_id[keep], np.arange(40))
    assert all((np.diff(ci[rp[r]:rp[r + 1]].astype(np.int64)) >= 0).all() for r in range(40))


def test_entry_points_are_declared():
    header = open(os.path.join(ROOT, "include", "f2v.h")).read()
    for name in ("f2v_components", "f2v_spanning_forest", "f2v_edge_split_connected", "f2v_subgraph"):
        assert name in _lib.SIGNATURES and "F2V_API int %s(" % name in header
    for name in ("components", "spanning_forest", "subgraph", "largest_component"):
        assert callable(getattr(F.Engine, name))
    assert C.sizeof(_lib.ComponentsInfo) == 40 and C.sizeof(_lib.ForestInfo) == 32


def test_cli_help_and_refusals(tmp_path):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-components" in r.stdout and "-holdout-keep" in r.stdout and "anchor | forest" in r.stdout
    mtx = golden_graph_path("karate.mtx")
    r = subprocess.run([CLI, "-input", mtx, "-holdout", "0.3", "-holdout-keep", "tree"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-holdout-keep must be" in r.stdout, r.stdout
    r = subprocess.run([CLI, "-input", mtx, "-holdout-keep", "forest"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-holdout-keep needs -holdout" in r.stdout, r.stdout
    r = subprocess.run([CLI, "-input", mtx, "-components", "2"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-components must be" in r.stdout, r.stdout


KERNELS = ["cc_iota_kernel", "cc_hook_kernel", "cc_jump_kernel", "cc_size_kernel", "cc_stat_kernel", "cc_edges_kernel", "forest_key_kernel", "forest_pair_kernel",
           "forest_hook_kernel", "forest_mark_kernel", "sub_count_kernel", "sub_fill_kernel", "held_forest_count_kernel", "held_forest_fill_kernel"]
TU = '#include "f2v_components.hip.h"\n#include "f2v_heldout.hip.h"\n'


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "components_isa.hip"), str(tmp_path / "components_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


# ---- GPU: components -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", GRAPHS)
def test_components_equal_the_restatement(name):
    want = comps(name)
    a, b = F.Engine(*graph(name), 4), F.Engine(*graph(name), 4)
    try:
        for eng in (a, a, b):  # a second call and a second handle
            labels, info = eng.components(details=True)
            assert labels.dtype == info.sizes.dtype == np.uint32
            assert np.array_equal(labels, want["labels"]) and np.array_equal(info.sizes, want["sizes"])
            assert {k: getattr(info, k) for k in R.COMPONENT_COUNTERS} == {k: want[k] for k in R.COMPONENT_COUNTERS}
            assert info.seconds > 0 and eng.last_components_seconds == info.seconds
        assert np.array_equal(a.components(), want["labels"])
    finally:
        a.close()
        b.close()


# ---- GPU: spanning forests -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", GRAPHS)
def test_forests_equal_the_restatement(name):
    c = comps(name)
    n = len(c["labels"])
    a, b = F.Engine(*graph(name), 4), F.Engine(*graph(name), 4)
    try:
        assert a.get_param("forest_key_bits") == 64
        for bits in (64, 2, 1):
            for eng in (a, b):
                eng.set_param("forest_key_bits", bits)
            for seed in (1, 2):
                for greatest in (False, True):
                    wu, wv = forest(name, seed, greatest, bits)
                    for eng in (a, a, b):
                        u, v, info = eng.spanning_forest(seed=seed, greatest=greatest, details=True)
                        assert u.dtype == v.dtype == np.uint32 and np.array_equal(u, wu) and np.array_equal(v, wv), (name, bits, seed, greatest)
                        assert len(u) == n - c["components"] == info.forest_edges and info.components == c["components"] and info.edges == c["edges"]
                        assert info.rounds >= 1 and len(info.round_seconds) == info.rounds
    finally:
        a.close()
        b.close()


# ---- GPU: the connected split --------------------------------------------------------------------------------------------------------
def same_split(got, want):
    return all(np.array_equal(getattr(got, k), want[k]) and getattr(got, k).dtype == np.uint32 for k in ARRAYS) and \
        all(getattr(got.info, k) == want[k] for k in H.SPLIT_COUNTERS)


@gpu
@pytest.mark.parametrize("name", GRAPHS)
def test_connected_split_equals_the_restatement(name):
    full = comps(name)["labels"]
    a, b = F.Engine(*graph(name), 4), F.Engine(*graph(name), 4)
    try:
        fu, fv = a.spanning_forest(seed=1, greatest=True)
        tree = set(zip(fu.tolist(), fv.tolist()))
        for frac in (0.0, 0.3, 0.9):
            for ratio in (0, 2):
                want = connected(name, frac, ratio)
                for eng in (a, a, b):
                    got = eng.edge_split(frac=frac, seed=1, ratio=ratio, details=True, keep="forest")
                    assert same_split(got, want), (name, frac, ratio, got.info, {k: want[k] for k in H.SPLIT_COUNTERS})
                held = set(zip(got.held_u.tolist(), got.held_v.tolist()))
                assert not held & tree and (frac > 0) == (len(held) > 0)
                cand = H.split(*graph(name), frac, seed=1, ratio=0) if name == "karate" else None
                if cand is not None:  # the anchors' held pairs are candidates too; the forest's come from the same candidates
                    assert got.info.candidates_held == cand["candidates_held"]
                train = F.Engine(got.rowptr, got.colids, 4)
                try:
                    assert np.array_equal(train.components(), full)  # the training graph has the full graph's components
                finally:
                    train.close()
        a.set_param("forest_key_bits", 1)  # the knob moves the forest, never the candidates
        low = a.edge_split(frac=0.3, seed=1, ratio=0, details=True, keep="forest")
        assert low.info.candidates_held == connected(name, 0.3, 0)["candidates_held"] and same_split(low, R.split_connected(*graph(name), 0.3, 1, 0, bits=1))
    finally:
        a.close()
        b.close()


@gpu
@pytest.mark.parametrize("name", ["karate", "cora"])
def test_keep_anchor_is_the_split_as_before(name):
    eng = F.Engine(*graph(name), 4)
    try:
        for frac, ratio in ((0.3, 1), (0.9, 2)):
            want = H.split(*graph(name), frac, seed=1, ratio=ratio)
            eng.edge_split(frac=frac, ratio=ratio, keep="forest")  # the forest call in between leaves the anchor path alone
            for got in (eng.edge_split(frac=frac, ratio=ratio, details=True), eng.edge_split(frac=frac, ratio=ratio, details=True, keep="anchor")):
                assert same_split(got, want), (name, frac, ratio)
        with pytest.raises(ValueError):
            eng.edge_split(keep="tree")
    finally:
        eng.close()


# ---- GPU: subgraphs ------------------------------------------------------------------------------------------------------------------
def same_subgraph(got, want):
    return all(np.array_equal(g, w) and g.dtype == np.uint32 for g, w in zip(got, want))


@gpu
@pytest.mark.parametrize("name", ["cora", "pieces"])
def test_subgraphs_equal_the_restatement(name):
    rowptr, colids = graph(name)
    c = comps(name)
    n = len(c["labels"])
    eng, other = F.Engine(rowptr, colids, 4), F.Engine(rowptr, colids, 4)
    try:
        largest = c["labels"] == c["largest_label"]
        want = R.subgraph(rowptr, colids, largest)
        for e in (eng, eng, other):
            assert same_subgraph(e.largest_component(), want)
        assert same_subgraph(eng.subgraph(np.flatnonzero(largest)), want)  # an id list
        assert len(want[2]) == c["largest"] and eng.last_subgraph_seconds > 0
        sub = F.Engine(want[0], want[1], 4)
        try:
            labels, info = sub.components(details=True)
            assert info.components == 1 and info.largest == c["largest"] and not labels.any()
        finally:
            sub.close()
        everything = eng.subgraph(np.ones(n, dtype=bool))
        assert np.array_equal(everything.rowptr, rowptr) and np.array_equal(everything.colids, colids) and np.array_equal(everything.new_id, np.arange(n))
        nothing = eng.subgraph(np.zeros(n, dtype=bool))
        assert np.array_equal(nothing.rowptr, [0]) and len(nothing.colids) == len(nothing.ids) == 0 and (nothing.new_id == R.DROPPED).all()
        for v in ((5, 10, 400) if name == "pieces" else (0, 1)):  # a single vertex: only its self-loops stay
            assert same_subgraph(eng.subgraph([v]), R.subgraph(rowptr, colids, np.arange(n) == v)), v
        mask = np.random.default_rng(3).random(n) < 0.5
        assert same_subgraph(eng.subgraph(mask), R.subgraph(rowptr, colids, mask))
    finally:
        eng.close()
        other.close()


# ---- GPU: nothing else moves ---------------------------------------------------------------------------------------------------------
@gpu
def test_the_calls_touch_neither_the_matrix_nor_the_rand_stream():
    rowptr, colids = graph("karate")
    a, b = F.Engine(rowptr, colids, 16), F.Engine(rowptr, colids, 16)
    try:
        for e in (a, b):
            e.srand(5)
            e.init_embeddings(0)
            e.train(5, 2, 16, 5, 0.02)
        a.components(details=True)
        a.spanning_forest(seed=3, greatest=False)
        a.edge_split(frac=0.3, keep="forest")
        a.largest_component()
        assert np.array_equal(a.get_embeddings(), b.get_embeddings())
        assert [a.rand_index(1000) for _ in range(8)] == [b.rand_index(1000) for _ in range(8)]
        a.train(5, 5, 16, 5, 0.02)
        b.train(5, 5, 16, 5, 0.02)
        assert np.array_equal(a.get_embeddings(), b.get_embeddings())
    finally:
        a.close()
        b.close()


# ---- GPU: refusals -------------------------------------------------------------------------------------------------------------------
@gpu
def test_calling_conventions_and_refusals():
    rowptr, colids = graph("karate")
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 4)
    L, h, EINVAL = eng._L, eng._h, _lib.F2V_EINVAL
    message = lambda: L.f2v_last_error().decode()
    u32 = lambda a: a.ctypes.data_as(_lib.u32p)
    try:
        labels, cinfo = np.zeros(n, dtype=np.uint32), _lib.ComponentsInfo()
        assert L.f2v_components(h, u32(labels), None, C.byref(cinfo)) == 0 and cinfo.components == 1  # sizes_out may be NULL
        assert L.f2v_components(h, None, None, C.byref(cinfo)) == EINVAL and L.f2v_components(h, u32(labels), None, None) == EINVAL
        assert L.f2v_components(None, u32(labels), None, C.byref(cinfo)) == EINVAL

        count, finfo = C.c_uint64(0xDEAD), _lib.ForestInfo()
        assert L.f2v_spanning_forest(h, 1, 1, None, None, 0, C.byref(count), C.byref(finfo)) == 0 and count.value == n - 1 == finfo.forest_edges  # count only
        u, v = np.full(n, 77, dtype=np.uint32), np.full(n, 77, dtype=np.uint32)
        assert L.f2v_spanning_forest(h, 1, 1, u32(u), u32(v), n, C.byref(count), None) == 0 and (u[n - 1:] == 77).all() and (u[:n - 1] < v[:n - 1]).all()
        u[:], count.value = 77, 0xDEAD
        assert L.f2v_spanning_forest(h, 1, 1, u32(u), u32(v), n - 2, C.byref(count), None) == EINVAL and count.value == n - 1 and (u == 77).all() and "arrays hold" in message()
        assert L.f2v_spanning_forest(h, 1, 2, None, None, 0, C.byref(count), None) == EINVAL and "greatest" in message()
        assert L.f2v_spanning_forest(h, 1, 1, u32(u), None, n, C.byref(count), None) == EINVAL and "together" in message()
        assert L.f2v_spanning_forest(h, 1, 1, None, None, 0, None, None) == EINVAL
        for bits in (0, 65):
            with pytest.raises(F.F2VError, match="forest_key_bits must be 1..64"):
                eng.set_param("forest_key_bits", bits)
        assert eng.get_param("forest_key_bits") == 64

        want = connected("karate", 0.3, 1)
        sizes = (want["train_nnz"], want["held"], want["negatives"])

        def raw(arrays, caps, counts=True):
            c = [C.c_uint64(0xDEAD) for _ in range(3)]
            refs = [C.byref(x) if counts else None for x in c]
            ptr = lambda a: u32(a) if a is not None else None
            rc = L.f2v_edge_split_connected(h, 0.3, 1, 1, ptr(arrays[0]), ptr(arrays[1]), caps[0], ptr(arrays[2]), ptr(arrays[3]), caps[1], ptr(arrays[4]), ptr(arrays[5]),
                                            caps[2], *refs, None)
            return rc, tuple(x.value for x in c)

        none = [None] * 6
        assert raw(none, (0, 0, 0)) == (0, sizes)
        fresh = lambda: [np.full(n + 1, 77, dtype=np.uint32)] + [np.full(s, 77, dtype=np.uint32) for s in (sizes[0], sizes[1], sizes[1], sizes[2], sizes[2])]
        for short in range(3):  # a capacity too small: F2V_EINVAL with the counts written, nothing else
            arrays = fresh()
            rc, counts = raw(arrays, tuple(s - (i == short) for i, s in enumerate(sizes)))
            assert rc == EINVAL and counts == sizes and all((a == 77).all() for a in arrays) and "f2v_edge_split_connected" in message()
        for k in (0, 3, 5):
            partial = fresh()
            partial[k] = None
            assert raw(partial, sizes)[0] == EINVAL and "together" in message()
        assert raw(none, (0, 0, 0), counts=False)[0] == EINVAL

        keep = np.ones(n, dtype=np.uint8)
        k8 = keep.ctypes.data_as(_lib.u8p)
        rows, nnz = C.c_uint32(0xDEAD), C.c_uint64(0xDEAD)
        assert L.f2v_subgraph(h, k8, None, None, 0, None, C.byref(rows), C.byref(nnz)) == 0 and (rows.value, nnz.value) == (n, len(colids))  # count only
        rp, ci = np.full(n + 1, 77, dtype=np.uint32), np.full(len(colids), 77, dtype=np.uint32)
        rows.value, nnz.value = 0xDEAD, 0xDEAD
        assert L.f2v_subgraph(h, k8, u32(rp), u32(ci), len(colids) - 1, None, C.byref(rows), C.byref(nnz)) == EINVAL and (rows.value, nnz.value) == (n, len(colids))
        assert (rp == 77).all() and (ci == 77).all() and "colids_out holds" in message()
        assert L.f2v_subgraph(h, k8, u32(rp), None, len(colids), None, C.byref(rows), C.byref(nnz)) == EINVAL and "together" in message()
        assert L.f2v_subgraph(h, None, None, None, 0, None, C.byref(rows), C.byref(nnz)) == EINVAL
        assert L.f2v_subgraph(h, k8, None, None, 0, None, None, C.byref(nnz)) == EINVAL
        assert L.f2v_subgraph(h, k8, u32(rp), u32(ci), len(colids), None, C.byref(rows), C.byref(nnz)) == 0 and np.array_equal(rp, rowptr) and np.array_equal(ci, colids)  # new_id_out may be NULL
        with pytest.raises(ValueError):
            eng.subgraph([n])
        with pytest.raises(ValueError):
            eng.subgraph(np.ones(n + 1, dtype=bool))
    finally:
        eng.close()
    shuffled = colids.copy()
    shuffled[rowptr[0]:rowptr[1]] = shuffled[rowptr[0]:rowptr[1]][::-1]
    eng = F.Engine(rowptr, shuffled, 4)
    try:
        for call, who in ((eng.components, "f2v_components"), (eng.spanning_forest, "f2v_spanning_forest"),
                          (lambda: eng.edge_split(keep="forest"), "f2v_edge_split_connected")):
            with pytest.raises(F.F2VError, match=who + ": the CSR's column ids are not ascending") as e:
                call()
            assert e.value.code == _lib.F2V_EINVAL
    finally:
        eng.close()


# ---- GPU: the command line -----------------------------------------------------------------------------------------------------------
@gpu
def test_cli_components_and_holdout_keep(tmp_path):
    mtx = golden_graph_path("cora.mtx")
    base = [CLI, "-input", mtx, "-iter", "1", "-dim", "8", "-batch", "256", "-option", "5", "-seed", "1", "-notext", "1", "-binout", "1"]
    out = {}
    for keep in ("anchor", "forest"):
        d = tmp_path / keep
        d.mkdir()
        extra = ["-components", "1"] + (["-holdout-keep", "forest"] if keep == "forest" else [])
        r = subprocess.run(base + ["-holdout", "0.3", "-output", str(d) + "/"] + extra, capture_output=True, text=True, cwd=d, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"^Held-out link prediction\(l2\): (\d+) edges :AUC: (\S+) AP: (\S+)$", r.stdout, re.M)
        c = re.search(r"^Components: (\d+) Largest: (\d+) Isolated: (\d+)$", r.stdout, re.M)
        assert m and c, r.stdout
        out[keep] = (int(m.group(1)), tuple(int(x) for x in c.groups()), d)
    want = connected("cora", 0.3, 1)
    assert out["forest"][0] == want["held"] > out["anchor"][0] == H.split(*graph("cora"), 0.3, seed=1, ratio=1)["held"]
    cc = comps("cora")
    assert out["forest"][1] == (78, 2485, cc["isolated"])  # the forest split's training graph: the components of cora itself
    d = out["forest"][2]
    held = [p for p in os.listdir(d) if p.endswith(".held")]
    ccs = [p for p in os.listdir(d) if p.endswith(".cc")]
    assert len(held) == 1 and len(ccs) == 1
    lines = np.loadtxt(str(d / held[0]), dtype=np.int64).reshape(-1, 3)
    assert np.array_equal(lines[:, 0] - 1, np.concatenate([want["held_u"], want["neg_u"]])) and np.array_equal(lines[:, 1] - 1, np.concatenate([want["held_v"], want["neg_v"]]))
    assert np.array_equal(lines[:, 2], np.concatenate([np.ones(want["held"]), np.zeros(want["negatives"])]))
    table = np.loadtxt(str(d / ccs[0]), dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(table[:, 0], np.arange(len(cc["labels"]))) and np.array_equal(table[:, 1], cc["labels"])
