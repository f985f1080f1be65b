"""Neighbourhood scores of pairs (include/f2v.h: f2v_pair_neighbourhood; Engine.pair_neighbourhood / heldout_baselines; bin/Force2Vec
-holdout-baselines): common neighbours, Jaccard, Adamic-Adar, resource allocation and preferential attachment of a pair on the GPU.

Host tests (no GPU): the restatement (tests/neighbourhood_ref.py) against networkx, its bit-for-bit properties and hand-written values,
that the definition's piece order shows in the bits, and the declarations.  -m gpu: the engine against the restatement, bit for bit
(uint64 views), on karate, on a graph with every irregularity of a CSR, on rows around the piece length, across chunks and past the
grid cap; the held-out baselines end to end; that the call leaves the handle's other state alone; its refusals; the CLI."""
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
import neighbourhood_ref as R
import scale_graphs as SG
from exact_ref import flog
from test_gather_isa import FLAGS, HIPCC, function
from test_linkpairs import both, csr
from test_logreg import spills

gpu = pytest.mark.gpu
CLI = os.path.join(ROOT, "bin", "Force2Vec")
KINDS = R.KINDS
ARRAYS = ("rowptr", "colids", "held_u", "held_v", "neg_u", "neg_v")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def all_equal(got, want):
    return set(got) == set(want) and all(same_bits(got[k], want[k]) for k in want)


# ---- the graphs ------------------------------------------------------------------------------------------------------------------------
def mixed():
    """n = 300, of the kind of test_heldout.mixed.  Vertices 0..17 are a core written out by hand, without a nonzero to the rest:
         0: 1 2 3      1: 0 2      2: 0 1 7      3: 0 7      7: 2 3 7 9 9 (a self-loop, a duplicated nonzero)      5: isolated
         9: 7 10 12 13 14 15      10: 9      12: 9 13 14 15 16 17      13, 14, 15: 9 12      16, 17: 12
         4: 6 8 11      8: 4 6 11      6: nothing      11: 4   (4 -> 6, 8 -> 6 and 8 -> 11 are stored in one direction only: d(6) = 0, d(11) = 1)
    so N(7) = {2, 3, 9}, d(7) = 3, d(9) = 6, d(12) = 6.  Vertices 40..299: seeded random pairs, about six nonzeros a vertex."""
    n, rng = 300, np.random.default_rng(11)
    plain = np.arange(40, n)
    und = {(int(min(a, b)), int(max(a, b))) for a, b in zip(rng.choice(plain, 3 * n), rng.choice(plain, 3 * n)) if a != b}
    core = {(0, 1), (0, 2), (0, 3), (1, 2), (2, 7), (3, 7), (7, 9), (9, 10), (9, 12), (9, 13), (9, 14), (9, 15), (12, 13), (12, 14), (12, 15), (12, 16), (12, 17)}
    one_way = [(7, 7), (7, 9), (4, 6), (4, 8), (8, 4), (4, 11), (11, 4), (8, 6), (8, 11)]
    return csr(n, both(sorted(und | core)) + one_way)


HUB_N = 8192
BIG, ROWS, TIE, SHARE, AUX, LEAF = 0, {1: 1023, 2: 1024, 3: 1025, 4: 2048, 5: 2049}, (6, 7), (8, 9), range(10, 16), 16
SHARED = range(6000, 8100)  # the 2100 common neighbours of SHARE: d(w) = 2 + w % 7


def hub():
    """n = 8192.  Vertex 0: 5000 leaves (100..5099).  Vertices 1..5: rows of 1023, 1024, 1025, 2048 and 2049 leaves from 3900 on, so
    that each shares its leaves below 5100 with vertex 0 and the leaves' degrees vary from 2 to 7.  6 and 7: two rows of 1500 leaves
    (2000.. and 2500..): equal lengths.  8 and 9 share the 2100 leaves 6000..8099; leaf w is also tied to w % 7 of the vertices 10..15, so
    d(w) = 2 + w % 7; 9 has 50 more leaves, so 8 is S: three pieces.  16 is a leaf of one nonzero (150, a leaf of vertex 0)."""
    und = {(BIG, w) for w in range(100, 5100)}
    for h, d in ROWS.items():
        und |= {(h, w) for w in range(3900, 3900 + d)}
    und |= {(TIE[0], w) for w in range(2000, 3500)} | {(TIE[1], w) for w in range(2500, 4000)}
    for w in SHARED:
        und |= {(SHARE[0], w), (SHARE[1], w)} | {(AUX[k], w) for k in range(w % 7)}
    und |= {(SHARE[1], w) for w in range(5950, 6000)} | {(LEAF, 150)}
    return csr(HUB_N, both(sorted(und)))


HUB_PAIRS = [(h, BIG) for h in ROWS] + [(BIG, h) for h in ROWS] + [(1, 5), (2, 4), (4, 5), (5, 4), (3, 2), TIE, TIE[::-1], (BIG, LEAF), (LEAF, BIG), SHARE, SHARE[::-1],
                                                                 (BIG, BIG), (4, 4), (8, 8), (9, 9), (BIG, 8), (10, 11), (15, 10), (150, 16), (6000, 6007), (100, 8191)]


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in ("karate", "cora"):
        return F.read_mtx(golden_graph_path(name + ".mtx"))
    if name == "medium":
        return SG.graph("medium")
    return {"mixed": mixed, "hub": hub}[name]()


@functools.lru_cache(maxsize=None)
def restated(name):
    """shared, never modified"""
    return R.Graph(*graph(name))


def every_pair(n):
    u, v = np.divmod(np.arange(n * n, dtype=np.int64), n)
    return u.astype(np.uint32), v.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def every_score(name):
    """the restated scores of all n x n ordered pairs, u == v included: shared, never modified"""
    g = restated(name)
    return g.scores(*every_pair(g.n))


def distance_two(name, count, seed):
    """`count` pairs (u, x): x a neighbour of a neighbour of u, both nonzeros drawn at random (x == u happens and is legal)"""
    rowptr, colids = (np.asarray(a, dtype=np.int64) for a in graph(name))
    rng = np.random.default_rng(seed)
    e = rng.integers(0, len(colids), count)
    u, w = np.searchsorted(rowptr, e, side="right") - 1, colids[e]
    deg = rowptr[w + 1] - rowptr[w]
    assert (deg > 0).all()  # every generator here stores an edge in both directions
    x = colids[rowptr[w] + rng.integers(0, 1 << 40, count) % deg]
    return u.astype(np.uint32), x.astype(np.uint32)


def half_and_half(name, count, seed):
    """half at distance two, half random"""
    n = len(graph(name)[0]) - 1
    u, v = distance_two(name, count // 2, seed)
    rng = np.random.default_rng(seed + 1)
    ru, rv = rng.integers(0, n, count - len(u)), rng.integers(0, n, count - len(u))
    return np.concatenate([u, ru.astype(np.uint32)]), np.concatenate([v, rv.astype(np.uint32)])


# ---- host: the restatement against networkx ---------------------------------------------------------------------------------------------
def nx_graph(name):
    nx = pytest.importorskip("networkx")
    g, G = restated(name), nx.Graph()
    G.add_nodes_from(range(g.n))
    for u in range(g.n):
        G.add_edges_from((u, w) for w in set(g.row(u)[0]) if w != u)
    return nx, G


@pytest.mark.parametrize("name", ["karate", "cora"])
def test_restatement_equals_networkx(name):
    """CN, Jaccard and PA exactly.  AA and RA within 1e-12 relative: a term differs by at most about 3 * 2^-53 (flog and libm's log
    within an ulp each, one division), k positive terms added in another order by at most (k - 1) * 2^-53 relative, k <= 168 on cora:
    below 2e-14."""
    nx, G = nx_graph(name)
    g = restated(name)
    if name == "karate":
        u, v = every_pair(g.n)
        u, v = u[u != v], v[u != v]
        assert len(u) == 34 * 33
    else:
        du, dv = distance_two("cora", 1500, 3)
        rng = np.random.default_rng(4)
        u, v = np.concatenate([du, rng.integers(0, g.n, 500).astype(np.uint32)]), np.concatenate([dv, rng.integers(0, g.n, 500).astype(np.uint32)])
        u, v = u[u != v], v[u != v]
    got = g.scores(u, v)
    pairs = list(zip(u.tolist(), v.tolist()))
    with_common = int((got["cn"] > 0).sum())
    print("%s: %d of %d pairs have a common neighbour" % (name, with_common, len(pairs)))
    assert 2 * with_common >= len(pairs)
    assert got["cn"].tolist() == [float(len(list(nx.common_neighbors(G, a, b)))) for a, b in pairs]
    assert got["jaccard"].tolist() == [p for _, _, p in nx.jaccard_coefficient(G, pairs)]
    assert got["pa"].tolist() == [float(p) for _, _, p in nx.preferential_attachment(G, pairs)]
    worst = 0.0
    for kind, fn in (("aa", nx.adamic_adar_index), ("ra", nx.resource_allocation_index)):
        want = np.array([p for _, _, p in fn(G, pairs)])
        assert ((want == 0) == (got[kind] == 0)).all()
        rel = np.abs(got[kind] - want) / np.maximum(want, 1e-300)
        worst = max(worst, float(rel[want > 0].max()))
        assert (rel[want > 0] <= 1e-12).all(), (kind, rel.max())
    print("%s: largest relative difference of AA / RA from networkx %.3g" % (name, worst))


# ---- host: bit-for-bit properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karate", "mixed"])
def test_restatement_is_symmetric_and_knows_a_vertex_paired_with_itself(name):
    g, s = restated(name), every_score(name)
    n = g.n
    for kind in KINDS:
        m = s[kind].reshape(n, n)
        assert same_bits(m, m.T), kind
    diag = np.arange(n) * (n + 1)
    assert s["cn"][diag].tolist() == g.deg.astype(np.float64).tolist()                      # u == v: c = d(u)
    assert s["jaccard"][diag].tolist() == [1.0 if d else 0.0 for d in g.deg.tolist()]       # ... and Jaccard 1, or +0 for an isolated vertex
    assert not np.signbit(s["jaccard"]).any()
    assert s["pa"][diag].tolist() == (g.deg.astype(np.float64) ** 2).tolist()


def test_values_written_out_by_hand_on_mixed():
    g = restated("mixed")
    assert [int(g.deg[u]) for u in (0, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12)] == [3, 3, 2, 3, 0, 0, 3, 3, 6, 1, 6]
    f = lambda d: float(flog(np.array([float(d)]))[0])
    hand = {
        # N(0) = {1, 2, 3}, N(7) = {2, 3, 9}: W = {2, 3}, S = 0 (three nonzeros against five)
        (0, 7): (2, 2 / 4, 1.0 / f(3) + 1.0 / f(2), 1.0 / 3.0 + 1.0 / 2.0, 9.0),
        # the duplicated nonzero: S = 7 (five nonzeros against six) walks 2, 3, 7, 9, 9: 9 counts once.  d(9) = 6
        (7, 12): (1, 1 / 8, 1.0 / f(6), 1.0 / 6.0, 18.0),
        (7, 10): (1, 1 / 3, 1.0 / f(6), 1.0 / 6.0, 3.0),
        # the self-loop: 7 is no neighbour of itself, d(7) = 3, and as a common neighbour of 2 and 3 it counts with d = 3
        (7, 7): (3, 1.0, (1.0 / f(3) + 1.0 / f(2)) + 1.0 / f(6), (1.0 / 3.0 + 1.0 / 2.0) + 1.0 / 6.0, 9.0),
        (2, 3): (2, 2 / 3, 1.0 / f(3) + 1.0 / f(3), 1.0 / 3.0 + 1.0 / 3.0, 6.0),
        # the isolated vertex, alone and against a vertex without neighbours of its own
        (5, 0): (0, 0.0, 0.0, 0.0, 0.0),
        (5, 5): (0, 0.0, 0.0, 0.0, 0.0),
        (5, 6): (0, 0.0, 0.0, 0.0, 0.0),
        # nonzeros stored in one direction only: N(4) = {6, 8, 11}, N(8) = {4, 6, 11}, N(6) = {}, N(11) = {4}.  W(4, 8) = {6, 11}: d(6) = 0
        # adds nothing to either sum, d(11) = 1 adds nothing to AA and 1.0 to RA
        (4, 8): (2, 2 / 4, 0.0, 1.0, 9.0),
        (4, 6): (0, 0.0, 0.0, 0.0, 0.0),
        (11, 8): (1, 1 / 3, 1.0 / f(3), 1.0 / 3.0, 3.0),
        (6, 11): (0, 0.0, 0.0, 0.0, 0.0),
    }
    for (u, v), want in hand.items():
        for a, b in ((u, v), (v, u)):
            got = g.pair(a, b)
            assert same_bits(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64)), ((a, b), got, want)


def test_the_piece_order_shows_in_the_bits():
    """8 and 9 of `hub` share 2100 neighbours of degree 2 + w % 7 and S = 8 spans three pieces: under the definition both sums differ
    in bits from one plain sequential sum, so the GPU comparison can tell the two orders apart."""
    g = restated("hub")
    assert g.s_and_l(*SHARE) == SHARE and g.s_and_l(*SHARE[::-1]) == SHARE and g.rowptr[9] - g.rowptr[8] == 2100
    assert all(g.deg[w] == 2 + w % 7 for w in SHARED)
    pieces, plain = g.pair(*SHARE), g.pair(*SHARE, piece=1 << 40)
    assert pieces[0] == plain[0] == 2100
    for k in (2, 3):
        assert np.float64(pieces[k]).tobytes() != np.float64(plain[k]).tobytes(), (k, pieces[k], plain[k])
        assert abs(pieces[k] - plain[k]) <= 1e-12 * plain[k]


def test_hub_has_the_rows_the_issue_names():
    g = restated("hub")
    length = np.diff(g.rowptr)
    assert [int(length[h]) for h in ROWS] == list(ROWS.values()) and length[BIG] == 5000 and length[TIE[0]] == length[TIE[1]] == 1500
    assert g.s_and_l(*TIE) == TIE and g.s_and_l(*TIE[::-1]) == TIE                # the tie goes to the lower id
    assert length[LEAF] == 1 and g.pair(BIG, LEAF)[0] == 1 and g.s_and_l(BIG, LEAF) == (LEAF, BIG)
    assert all(g.s_and_l(h, BIG) == (h, BIG) and g.pair(h, BIG)[0] == min(d, 1200) for h, d in ROWS.items())  # the leaves 3900 .. 5099
    assert g.pair(4, 5)[0] == 2048 and g.pair(10, 11)[0] == 1500 and g.pair(*TIE)[0] == 1000


# ---- host: declarations ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared():
    assert "f2v_pair_neighbourhood" in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "f2v.h")).read()
    assert re.search(r"F2V_API int f2v_pair_neighbourhood\(f2v_handle h, const uint32_t \*u_ids, const uint32_t \*v_ids, uint64_t m, uint32_t kinds,", hdr)
    for name, bit in zip(("COMMON", "JACCARD", "ADAMIC_ADAR", "RESOURCE", "PREFERENTIAL", "ALL"), (1, 2, 4, 8, 16, 31)):
        assert re.search(r"#define F2V_NB_%s %du\b" % (name, bit), hdr), name
    assert "#define F2V_NB_PIECE 1024" in hdr
    for name in ("pair_neighbourhood", "heldout_baselines"):
        assert callable(getattr(F.Engine, name))


def test_cli_help_and_refusal(tmp_path):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert "-holdout-baselines" in r.stdout
    r = subprocess.run([CLI, "-input", golden_graph_path("karate.mtx"), "-holdout-baselines", "1"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-holdout-baselines" in r.stdout and "-holdout " in r.stdout, r.stdout


KERNELS = ["nb_degree_kernel", "nb_count_kernel", "nb_fill_kernel", "nb_pair_kernelILb0EE", "nb_pair_kernelILb1EE", "nb_finish_kernel"]
TU = '#include "f2v_neighbourhood.hip.h"\n' + "".join("template __global__ void f2v::nb_pair_kernel<%s>(const f2v::NbArgs);\n" % b for b in ("false", "true"))


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "neighbourhood_isa.hip"), str(tmp_path / "neighbourhood_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def raw(eng, u, v, kinds, spare=1):
    """the C call itself into a buffer of `spare` arrays more than the kinds need, filled with a pattern -> (arrays [kinds, m], the spare part)"""
    u, v = np.ascontiguousarray(u, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)
    nk, m = bin(kinds).count("1"), len(u)
    buf = np.full((nk + spare) * m, 0xABCDABCDABCDABCD, dtype=np.uint64)
    _lib.check(eng._L.f2v_pair_neighbourhood(eng._h, u.ctypes.data_as(_lib.u32p), v.ctypes.data_as(_lib.u32p), m, kinds, buf.view(np.float64).ctypes.data_as(_lib.f64p), None), eng._L)
    return buf[:nk * m].view(np.float64).reshape(nk, m), buf[nk * m:]


@gpu
def test_karate_every_pair_every_kind_and_the_layout():
    u, v = every_pair(34)
    want = every_score("karate")
    eng = F.Engine(*graph("karate"), 4)
    try:
        got = eng.pair_neighbourhood(u, v)
        assert all_equal(got, want)
        assert eng.last_neighbourhood_seconds > 0
        for mask in (1, 2, 4, 8, 16, 2 | 8, 1 | 16, 31):
            names = [k for k in KINDS if R.BITS[k] & mask]
            arrays, spare = raw(eng, u, v, mask)
            assert all(same_bits(arrays[i], want[k]) for i, k in enumerate(names)), mask
            assert (spare == 0xABCDABCDABCDABCD).all(), mask   # nothing is written past the arrays asked for
        assert all_equal(eng.pair_neighbourhood(u, v, kinds=("ra", "jaccard")), {k: want[k] for k in ("ra", "jaccard")})
        assert same_bits(eng.pair_neighbourhood(u, v, kinds="pa")["pa"], want["pa"])
    finally:
        eng.close()


@gpu
def test_mixed_every_pair():
    u, v = every_pair(300)
    eng = F.Engine(*graph("mixed"), 4)
    try:
        assert all_equal(eng.pair_neighbourhood(u, v), every_score("mixed"))
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def hub_pairs(count=1000):
    """the pairs of HUB_PAIRS spread among random ones and pairs at distance two -> (u, v, the restated scores): shared, never modified"""
    u, v = half_and_half("hub", count - len(HUB_PAIRS), 8)
    at = np.sort(np.random.default_rng(9).choice(count, len(HUB_PAIRS), replace=False))
    uu, vv = np.empty(count, dtype=np.uint32), np.empty(count, dtype=np.uint32)
    rest = np.setdiff1d(np.arange(count), at)
    uu[at], vv[at] = np.array(HUB_PAIRS, dtype=np.uint32).T
    uu[rest], vv[rest] = u, v
    return uu, vv, restated("hub").scores(uu, vv)


@gpu
@pytest.mark.parametrize("spread", [1, 0])
def test_hub_rows_around_the_piece_length(spread):
    """S rows of 1023, 1024, 1025, 2048 and 2049 nonzeros, a tie of lengths, hub x leaf, the pair whose piece order shows, u == v on
    long rows: with the pieces as work items of their own (the default) and with one wavefront per pair."""
    u, v = np.array(HUB_PAIRS, dtype=np.uint32).T
    want = restated("hub").scores(u, v)
    eng = F.Engine(*graph("hub"), 4)
    try:
        eng.set_param("neighbourhood_spread", spread)
        got = eng.pair_neighbourhood(u, v)
        items = eng.get_param("last_neighbourhood_items")
        pieces = [-(-int(min(np.diff(restated("hub").rowptr)[[a, b]])) // 1024) for a, b in HUB_PAIRS]
        assert items == (sum(p for p in pieces if p > 1) if spread else 0)
        for kind in KINDS:
            bad = np.flatnonzero(got[kind].view(np.uint64) != want[kind].view(np.uint64))
            assert len(bad) == 0, (kind, [HUB_PAIRS[i] for i in bad[:5]], got[kind][bad[:5]], want[kind][bad[:5]])
        assert all_equal(eng.pair_neighbourhood(u, v, kinds=("cn", "jaccard")), {k: want[k] for k in ("cn", "jaccard")})  # no term is formed
    finally:
        eng.close()


@gpu
def test_the_chunk_size_changes_no_bit():
    u, v, want = hub_pairs()
    eng = F.Engine(*graph("hub"), 4)
    try:
        whole = eng.pair_neighbourhood(u, v)
        eng.set_param("pairs_chunk", 64)
        cut = eng.pair_neighbourhood(u, v)
        assert all_equal(whole, want) and all_equal(cut, want)
    finally:
        eng.close()


SCALE_CHUNK, SCALE_M = 65536, 3 * 65536 + 5
PER_PAIR_M = 2 * 2048 * 256 + 100  # two trips of the thread-per-pair launches (at most 2048 workgroups of 256 threads) and a third


@functools.lru_cache(maxsize=None)
def scale_set():
    """-> (u, v, the restated scores) of SCALE_M pairs of `medium`: shared, never modified"""
    u, v = half_and_half("medium", SCALE_M, 21)
    return u, v, restated("medium").scores(u, v)


def counted(name, u, v):
    """cn, jaccard and pa of many pairs by scipy.sparse and numpy: N(u) as a 0/1 matrix without its diagonal, c from the products of row
    slices, one rounded division and one rounded multiplication -- for sizes at which the per-pair restatement is too slow"""
    from scipy.sparse import csr_matrix
    g = restated(name)
    rows = np.repeat(np.arange(g.n), np.diff(g.rowptr))
    keep = rows != g.colids
    A = csr_matrix((np.ones(int(keep.sum()), dtype=np.int64), (rows[keep], g.colids[keep])), shape=(g.n, g.n))
    A.sum_duplicates()
    A.data[:] = 1
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    c = np.asarray(A[u].multiply(A[v]).sum(axis=1)).reshape(-1).astype(np.int64)
    du, dv = g.deg[u], g.deg[v]
    den = du + dv - c
    return {"cn": c.astype(np.float64), "jaccard": np.where(den > 0, c.astype(np.float64) / np.maximum(den, 1).astype(np.float64), 0.0),
            "pa": du.astype(np.float64) * dv.astype(np.float64)}


@gpu
def test_the_thread_per_pair_launches_stride_past_their_cap():
    """nb_count_kernel, nb_fill_kernel and nb_finish_kernel: more pairs in one chunk than two grids of them hold, one pair -- the hub
    of `medium` with itself -- with piece items.  The reference is the vectorised one, first shown equal to the restatement."""
    su, sv, swant = scale_set()
    assert all_equal(counted("medium", su, sv), {k: swant[k] for k in ("cn", "jaccard", "pa")})
    u, v = half_and_half("medium", PER_PAIR_M, 33)
    u[7] = v[7] = SG.MEDIUM_HUB
    want = counted("medium", u, v)
    eng = F.Engine(*graph("medium"), 4)
    try:
        eng.set_param("pairs_chunk", 1 << 21)
        assert all_equal(eng.pair_neighbourhood(u, v, kinds=("cn", "jaccard", "pa")), want)
        length = np.diff(restated("medium").rowptr)
        hub_pairs_here = int(((u == SG.MEDIUM_HUB) & (v == SG.MEDIUM_HUB)).sum())  # a walk hub - neighbour - hub is a pair at distance two
        assert 1024 < length[SG.MEDIUM_HUB] <= 2048 and np.sort(length)[-2] <= 1024 and hub_pairs_here >= 1
        assert eng.get_param("last_neighbourhood_items") == 2 * hub_pairs_here  # the hub's row alone has two pieces
        assert same_bits(eng.pair_neighbourhood(u, v, kinds="pa")["pa"], want["pa"])  # nb_finish_kernel alone
    finally:
        eng.close()


@gpu
def test_scale_across_chunks_and_past_the_grid_cap():
    """medium (n = 40000), "pairs_chunk" = 65536, 3 * 65536 + 5 pairs: three full chunks and one of five pairs; a full chunk is 65536
    work items for a grid of at most 8192 workgroups of four wavefronts: every wavefront takes a second trip."""
    assert SCALE_CHUNK >= 2 * 8192 * 4
    u, v, want = scale_set()
    assert 4 * int((want["cn"] > 0).sum()) >= len(u)
    eng = F.Engine(*graph("medium"), 4)
    try:
        eng.set_param("pairs_chunk", SCALE_CHUNK)
        got = eng.pair_neighbourhood(u, v)
        assert all_equal(got, want)
        eng.set_param("pairs_chunk", 1 << 20)
        assert all_equal(eng.pair_neighbourhood(u, v), want)
    finally:
        eng.close()


def same_ranking(a, b):
    return all(np.float64(getattr(a, k)).tobytes() == np.float64(getattr(b, k)).tobytes() for k in ("auc", "ap")) and \
        all(getattr(a, k) == getattr(b, k) for k in ("concordant", "tied", "positives", "negatives", "groups"))


@gpu
@pytest.mark.parametrize("keep", ["anchor", "forest"])
def test_cora_heldout_baselines_end_to_end(keep):
    full = F.Engine(*graph("cora"), 4)
    try:
        split = full.edge_split(0.3, keep=keep)
    finally:
        full.close()
    u, v = np.concatenate([split.held_u, split.neg_u]), np.concatenate([split.held_v, split.neg_v])
    y = np.concatenate([np.ones(len(split.held_u), dtype=np.uint8), np.zeros(len(split.neg_u), dtype=np.uint8)])
    want = R.scores(split.rowptr, split.colids, u, v)
    eng = F.Engine(split.rowptr, split.colids, 4)  # the training graph; no embeddings
    try:
        got = eng.heldout_baselines(split)
        assert list(got) == list(KINDS)
        for kind in KINDS:
            assert same_ranking(got[kind], eng.ranking(want[kind], y)), kind
        print("cora held-out baselines (frac 0.3, keep %s, %d edges): %s" % (keep, len(split.held_u), "  ".join("%s AUC %.4f AP %.4f" % (k, got[k].auc, got[k].ap) for k in KINDS)))
        two = eng.heldout_baselines(split, kinds=("pa", "cn"))
        assert list(two) == ["pa", "cn"] and same_ranking(two["cn"], got["cn"]) and same_ranking(two["pa"], got["pa"])
    finally:
        eng.close()


@gpu
def test_the_call_touches_nothing_else_of_the_handle():
    rowptr, colids = graph("karate")
    u, v = every_pair(34)
    want = every_score("karate")
    a, b = F.Engine(rowptr, colids, 16), F.Engine(rowptr, colids, 16)
    try:
        assert all_equal(a.pair_neighbourhood(u, v), want)  # before any embedding exists
        for e in (a, b):
            e.srand(5)
            e.init_embeddings(0)
            e.train(5, 2, 16, 5, 0.02)
        assert all_equal(a.pair_neighbourhood(u, v), want)
        a.train(5, 2, 16, 5, 0.02)
        b.train(5, 2, 16, 5, 0.02)
        assert np.array_equal(a.get_embeddings().view(np.uint32), b.get_embeddings().view(np.uint32))
        assert [a.rand_index(1000) for _ in range(8)] == [b.rand_index(1000) for _ in range(8)]
        first = a.pair_neighbourhood(u, v)
        a.kmeans(3)
        a.link_pairs()
        assert all_equal(a.pair_neighbourhood(u, v), first) and all_equal(first, want)
    finally:
        a.close()
        b.close()


@gpu
def test_refusals():
    rowptr, colids = graph("karate")
    eng = F.Engine(rowptr, colids, 4)
    L = eng._L
    ok = np.array([1, 2, 3], dtype=np.uint32)
    out = np.zeros(15)
    p = lambda a: a.ctypes.data_as(_lib.u32p)
    o = out.ctypes.data_as(_lib.f64p)
    try:
        for bad_u, bad_v in ((np.array([1, 34, 3], dtype=np.uint32), ok), (ok, np.array([1, 2, 34], dtype=np.uint32))):
            with pytest.raises(F.F2VError, match="names a vertex that is not one of the 34") as e:
                eng.pair_neighbourhood(bad_u, bad_v)
            assert e.value.code == _lib.F2V_EINVAL
        for kinds in (0, 32, 33):
            assert L.f2v_pair_neighbourhood(eng._h, p(ok), p(ok), 3, kinds, o, None) == _lib.F2V_EINVAL
            assert b"kinds" in L.f2v_last_error()
        for args in ((None, p(ok), 3, 31, o), (p(ok), None, 3, 31, o), (p(ok), p(ok), 3, 31, None)):
            assert L.f2v_pair_neighbourhood(eng._h, *args, None) == _lib.F2V_EINVAL
            assert b"null argument" in L.f2v_last_error()
        assert L.f2v_pair_neighbourhood(None, p(ok), p(ok), 3, 31, o, None) == _lib.F2V_EINVAL
        assert L.f2v_pair_neighbourhood(eng._h, None, None, 0, 31, None, None) == _lib.F2V_OK  # m = 0
        assert all(len(a) == 0 for a in eng.pair_neighbourhood([], []).values())
        with pytest.raises(ValueError):
            eng.pair_neighbourhood(ok, ok, kinds=("cn", "katz"))
        assert not out.any()
    finally:
        eng.close()
    shuffled = colids.copy()
    shuffled[rowptr[0]:rowptr[1]] = shuffled[rowptr[0]:rowptr[1]][::-1]
    descending = F.Engine(rowptr, shuffled, 4)
    try:
        with pytest.raises(F.F2VError, match="f2v_pair_neighbourhood: the CSR's column ids are not ascending") as e:
            descending.pair_neighbourhood([0], [1])
        assert e.value.code == _lib.F2V_EINVAL
    finally:
        descending.close()


@gpu
def test_cli_prints_the_engines_baselines(tmp_path):
    mtx = golden_graph_path("cora.mtx")
    common = [CLI, "-input", mtx, "-iter", "3", "-dim", "16", "-batch", "256", "-option", "5", "-seed", "1", "-holdout", "0.3", "-output", str(tmp_path) + "/"]
    with_flag = subprocess.run(common + ["-holdout-baselines", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    without = subprocess.run(common, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert with_flag.returncode == 0 and without.returncode == 0, with_flag.stdout + with_flag.stderr + without.stderr
    line = re.compile(r"^Held-out link prediction\(l2\): .*$", re.M)
    assert line.search(without.stdout) and line.search(with_flag.stdout).group(0) == line.search(without.stdout).group(0)
    assert "Held-out baseline" not in without.stdout
    full = F.Engine(*graph("cora"), 4)
    try:
        split = full.edge_split(0.3, seed=1, ratio=1)
    finally:
        full.close()
    eng = F.Engine(split.rowptr, split.colids, 4)
    try:
        want = eng.heldout_baselines(split)
    finally:
        eng.close()
    found = re.findall(r"^Held-out baseline\((\w+)\): (\d+) edges :AUC: (\S+) AP: (\S+)$", with_flag.stdout, re.M)
    assert [f[0] for f in found] == list(KINDS), with_flag.stdout
    for name, edges, auc, ap in found:
        assert int(edges) == len(split.held_u) and (float(auc), float(ap)) == (want[name].auc, want[name].ap), name
    after = with_flag.stdout.index("Held-out baseline(cn)")
    assert with_flag.stdout.index("Held-out link prediction(l2)") < after
