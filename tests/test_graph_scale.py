"""The integer graph and ranking calls where their grids stride and their scans carry (include/f2v.h: f2v_link_pairs, f2v_edge_split,
f2v_edge_split_connected, f2v_components, f2v_spanning_forest, f2v_subgraph, f2v_louvain, f2v_partition_agreement, f2v_modularity,
f2v_ranking, f2v_pair_scores).

The other test files compare these calls bit for bit with their restatements on graphs of at most 9000 vertices, where every launch
is below its cap on workgroups, every scan has one pass over its tile sums and no vertex sits on a boundary between two forms.  The
graphs of tests/scale_graphs.py are past those points: `thresholds` (one vertex on each side of every boundary), `medium` (n = 40000),
`large` (n = 262144 + 1500) and, for the components alone, n = 16384 * 256 + 1000.

Host tests: the graphs have the properties they are built for; CAPS restates every cap with the quantity that exceeds it (or says why
none does); the vectorised references equal the per-item restatements where both can run.  -m gpu: every array with array_equal, every
counter with ==, AUC and AP by their bytes.  No tolerance anywhere: everything is an integer or a bit pattern include/f2v.h defines."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import force2vec_amd as F
import components_ref as CR
import heldout_ref as HR
import kmeans_ref as KR
import louvain_ref as VR
import scale_graphs as S
from test_components import GRAPHS as CC_GRAPHS, comps as cc_comps, graph as cc_graph, same_subgraph
from test_heldout import N_ROWS, matrix, pairs, same_ranking, same_split, tied_scores
from test_linkpairs import csr, same as same_pairs
from test_louvain import FLOATS, INTEGERS, check_same as same_communities

gpu = pytest.mark.gpu
NAMES = ("thresholds", "medium", "large")
ENGINE_SOURCE = os.path.join(ROOT, "force2vec_amd", "csrc", "f2v_engine.hip")
RANK_SIZES = (65537, 262144 + 1025, 65536 * 256 + 1000)
PAIRS_M = 64 * 65536 + 100


# ---- host: the graphs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_graphs_are_ascending_symmetric_and_simple(name):
    rowptr, colids = S.graph(name)
    n = len(rowptr) - 1
    assert rowptr.dtype == colids.dtype == np.uint32 and rowptr[0] == 0 and rowptr[-1] == len(colids)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols = colids.astype(np.int64)
    assert (np.diff(cols)[rows[1:] == rows[:-1]] > 0).all()  # strictly ascending inside every row: no duplicate either
    assert (rows != cols).all() and np.array_equal(np.sort(rows * n + cols), np.sort(cols * n + rows))
    again = {"thresholds": S.thresholds, "medium": S.medium, "large": S.large_parts}[name].__wrapped__()
    assert np.array_equal(again[0], rowptr) and np.array_equal(again[1], colids)  # seeded: the same graph every time


def test_thresholds_has_a_vertex_on_each_side_of_every_boundary():
    rowptr, colids = S.thresholds()
    n, hubs = len(rowptr) - 1, len(S.hub_degrees())
    assert n == S.THRESHOLDS_N == 9300 and hubs == 16
    nu, p = S.degrees(rowptr, colids)
    total, capped = S.totals(rowptr, colids, 1)
    length = np.diff(rowptr.astype(np.int64))
    assert tuple(length[:hubs]) == tuple(nu[:hubs]) == tuple(p[:hubs]) == S.hub_degrees()  # all neighbours higher: p(u) is the degree
    assert tuple(total[:13]) == S.TOTALS == (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073)
    assert tuple(length[13:15]) == (512, 513) and {255, 256, 257} <= set(length[:hubs].tolist())
    assert all(colids[rowptr[h]] >= hubs for h in range(hubs))
    # the leaves: two or three hubs each and nothing else, so no higher neighbour, no negatives and no cap
    assert length[hubs:].max() <= 3 and length[hubs:].min() >= 1 and (p[hubs:] == 0).all() and (total[hubs:] == 0).all()
    assert not capped[:15].any() and not capped[hubs:].any()
    # the last hub: more than n / 2 neighbours, the cap A(u) / 2 binds
    assert nu[15] == S.CAPPED_DEGREE > n // 2 and capped[15] and total[15] == (n - 1 - S.CAPPED_DEGREE) // 2 == 2299
    assert int(capped.sum()) == 1
    # the three forms at the default "link_short_max" = 256: a wavefront up to 256, a table in LDS up to 3072, a table in the workspace
    assert sorted(total[(total > 0) & (total <= 256)].tolist()) == [1, 63, 64, 65, 255, 256]
    assert sorted(total[(total > 256) & (total <= 3072)].tolist()) == [257, 512, 513, 1023, 1024, 1025, 2299, 3071, 3072]
    assert total[total > 3072].tolist() == [3073]
    twice, capped2 = S.totals(rowptr, colids, 2)
    assert tuple(twice[:10]) == tuple(2 * t for t in S.TOTALS[:10]) and capped2[10:13].all()


def test_medium_is_past_the_strides_of_32768_and_16384():
    rowptr, colids = S.medium()
    n = len(rowptr) - 1
    nu, p = S.degrees(rowptr, colids)
    total, capped = S.totals(rowptr, colids, 1)
    assert n == S.MEDIUM_N == 40000 and 3.9 < len(colids) / n < 4.2
    assert nu[S.MEDIUM_HUB] >= S.MEDIUM_HUB_DEGREE == 2000 and p[S.MEDIUM_HUB] >= 2000 and np.delete(nu, S.MEDIUM_HUB).max() < 30
    assert not capped.any() and 256 < total[S.MEDIUM_HUB] <= 3072 and int((total > 0).sum()) > 8192 * 3
    assert (nu == 0).sum() > 100  # isolated vertices between the others


def test_large_is_past_the_second_pass_of_the_scans():
    rowptr, colids, alone = S.large_parts()
    n = len(rowptr) - 1
    nu, p = S.degrees(rowptr, colids)
    total, capped = S.totals(rowptr, colids, 1)
    length = np.diff(rowptr.astype(np.int64))
    lo, hi = S.LARGE_CHAIN
    assert n == S.LARGE_N == 262144 + 1500 and len(alone) == S.LARGE_ISOLATED == 3000 and (nu[alone] == 0).all() and int((nu == 0).sum()) == 3000
    assert all((colids[rowptr[v]:rowptr[v + 1]] == v + 1).any() for v in range(lo, hi - 1, 997)) and hi - lo == 40000
    assert length[S.LARGE_ROW] == S.LARGE_ROW_DEGREE == 700 and p[S.LARGE_ROW] == 0
    assert total[S.LARGE_HUB] == S.LARGE_HUB_DEGREE == 3100 > 3072 and not capped.any()
    assert int((total > 0).sum()) > 4 * 16384 and int(((total > 0) & (total <= 256)).sum()) > 4 * 16384
    c = S.components_fast(rowptr, colids)
    # 3000 isolated ids, the ascending path with its two hubs, and the stretches of the permuted path: 220642 ids in stretches of 998
    stretches = -(-(n - 3000 - 40000 - 2) // (S.LARGE_CUT + 1))
    assert (c["components"], c["isolated"], c["largest"], c["largest_label"]) == (3000 + 1 + stretches, 3000, 40002, S.LARGE_HUB) and stretches == 222
    assert c["rounds"] == 9  # the ids of a stretch lie all over the range: many rounds of hooking, long chains in between


def test_huge_is_past_the_cap_of_the_thread_grids():
    rowptr, colids = S.huge()
    n = len(rowptr) - 1
    assert n == S.HUGE_N == 16384 * 256 + 1000 and rowptr[-1] == len(colids) < 2 ** 31 and int((np.diff(rowptr.astype(np.int64)) == 0).sum()) == 3000


# ---- host: which cap every graph exceeds -----------------------------------------------------------------------------------------
def louvain_lists(name, short_max=32):
    """level 0 of f2v_louvain: the largest (class, form) list of the placement, and the number of nodes"""
    rowptr, _ = S.graph(name)
    n = len(rowptr) - 1
    length = np.diff(rowptr.astype(np.int64))
    cls = (KR.mix64(KR.mix64(np.uint64(1 + 0)) ^ np.arange(n, dtype=np.uint64)) % np.uint64(VR.PHASES)).astype(np.int64)
    short = np.bincount(cls[(length > 0) & (length <= short_max)], minlength=VR.PHASES)
    longer = np.bincount(cls[length > short_max], minlength=VR.PHASES)
    return int(short.max()), int(longer.max()), int(np.bincount(cls[length > 0], minlength=VR.PHASES).max())


def caps():
    """(kernels, the cap as f2v_engine.hip writes it, what a launch must exceed to stride or pass again, the quantity, the graph or input
    that brings it -- None: not reached at this n, with the reason)"""
    quantity = {}
    for name in NAMES:
        rowptr, colids = S.graph(name)
        total, _ = S.totals(rowptr, colids, 1)
        quantity[name] = dict(n=len(rowptr) - 1, drawing=int(((total > 0) & (total <= 256)).sum()), pieces=S.row_pieces(rowptr))
    n = {k: v["n"] for k, v in quantity.items()}
    short, longer, every = louvain_lists("large")
    return [
        ("link_count_kernel, link_positive_kernel", "rows = std::min((n + 3) / 4, 8192u)", 4 * 8192, n["medium"], "medium"),
        ("link_count_kernel, link_positive_kernel", "rows = std::min((n + 3) / 4, 8192u)", 2 * 4 * 8192, n["large"], "large"),
        ("held_anchor_kernel, held_count_kernel, held_forest_count_kernel, held_fill_kernel, held_forest_fill_kernel",
         "rows = std::min((n + 3) / 4, 8192u)", 4 * 8192, n["medium"], "medium"),
        ("sub_count_kernel, sub_fill_kernel", "rows = std::min((n + 3) / 4, 8192u)", 4 * 8192, n["medium"], "medium"),
        ("link_short_kernel", "dim3(std::min((a.count + 3) / 4, 16384u))", 4 * 16384, quantity["large"]["drawing"], "large"),
        ("cc_for_pieces: cc_hook_kernel, cc_edges_kernel, forest_key_kernel, forest_pair_kernel, forest_mark_kernel",
         "std::min<uint64_t>(((uint64_t)a.n + a.nitems + 3) / 4, 16384)", 4 * 16384, n["large"] + quantity["large"]["pieces"], "large"),
        ("modularity_kernel", "std::min((c->n + 3) / 4, 4096u)", 4 * 4096, n["medium"], "medium"),
        ("cc_grid: cc_iota_kernel, cc_jump_kernel, cc_size_kernel, cc_stat_kernel, forest_hook_kernel",
         "std::min<uint64_t>((threads + 255) / 256, 16384)", 256 * 16384, S.HUGE_N, "huge"),
        ("link_scan_top_kernel (link pairs, both splits, the subgraph)", "tiles = (uint32_t)(((uint64_t)n + kLinkScanTile - 1) / kLinkScanTile)",
         256 * 1024, n["large"], "large"),
        ("link_scan_top_kernel (the ranking)", "tiles = (mm + kLinkScanTile - 1) / kLinkScanTile", 256 * 1024, RANK_SIZES[1], "ranking"),
        ("rank_block_kernel", "dim3((blocks + 63u) / 64u)", 64 * 1024, RANK_SIZES[0], "ranking"),
        ("rank_key_kernel, rank_group_kernel", "grid(std::min((mm + 255u) / 256u, 65536u))", 256 * 65536, RANK_SIZES[2], "ranking"),
        ("pair_score_kernel", "grid(std::min((cm + 63u) / 64u, 65536u))", 64 * 65536, PAIRS_M, "pair scores"),
        ("louvain_symmetry_kernel", "std::min((c->n + 15) / 16, 16384u)", 16 * 16384, n["large"], "large"),
        ("louvain_degree_kernel", "rows16(std::max(1u, std::min((n + 15) / 16, 16384u)))", 16 * 16384, n["large"], "large"),
        ("louvain_qnum_kernel (level 0)", "std::min((a.N + 15) / 16, 16384u)", 16 * 16384, n["large"], "large"),
        ("louvain_scan_top_kernel (level 0: the renumbering of the kept communities)", "(count + kLouvainScanTile - 1) / kLouvainScanTile", 256 * 1024, n["large"],
         "large"),
        # a.count is the length of ONE list of the placement -- a class (of 8) and a form -- so about N / 8 at the most
        ("louvain_gather_kernel<0> (16 lanes a unit)", "dim3(std::min((a.count + 15) / 16, 16384u))", 16 * 16384, short,
         None, "a list holds one class of eight: %d units of `large`; it strides at n > 8 * 262144" % short),
        ("louvain_gather_kernel<1>, <2> (a workgroup a unit)", "dim3(std::min(a.count, 65536u))", 65536, max(longer, every),
         None, "with every unit a workgroup (\"louvain_short_max\" = 0) a list of `large` has %d units; it strides at n > 8 * 65536 such rows" % every),
        ("louvain_qnum_wide_kernel", "dim3(std::min(wide.count, 65536u))", 65536, longer, None, "the rows longer than 32 nonzeros of one class: %d in `large`" % longer),
    ]


def test_every_cap_is_exceeded_or_marked_out_of_reach():
    source = open(ENGINE_SOURCE).read()
    lines = source.split("\n")
    table = caps()
    for row in table:
        kernels, expression, bound, quantity, where = row[:5]
        at = [i + 1 for i, text in enumerate(lines) if expression in text]
        assert at, "f2v_engine.hip no longer writes: " + expression
        print("%-60s line %-16s needs > %-9d has %-9d %s" % (kernels[:60], ",".join(map(str, at)), bound, quantity, where or "NOT REACHED: " + row[5]))
        if where is None:
            assert quantity <= bound and row[5]
        else:
            assert quantity > bound, (kernels, quantity, bound)
    # every cap the engine puts on a launch of these calls is in the table: the sections from the link pairs to the subgraph
    first = next(i for i, text in enumerate(lines) if text.startswith("// ---- link prediction pairs"))
    last = next(i for i, text in enumerate(lines) if text.startswith("// ---- t-SNE layout"))
    assert first < last
    capped = [i for i in range(first, last) if "std::min" in lines[i] and re.search(r"\b(8192u|16384u|16384\)|65536u)", lines[i])]
    assert len(capped) >= 14
    for i in capped:
        assert any(row[1] in lines[i] for row in table), (i + 1, lines[i].strip())
    # the boundaries of `thresholds`
    kernels = "".join(open(os.path.join(ROOT, "force2vec_amd", "csrc", name)).read() for name in ("f2v_linkpairs.hip.h", "f2v_components.hip.h"))
    assert "kLinkLdsSlots = 8192;" in kernels and "kLinkWideThreads = 1024;" in kernels and "kCcPiece = 256;" in kernels
    slots = lambda total: max(2048, 1 << int(np.ceil(np.log2(2 * total + 2048))))  # link_slots of f2v_linkpairs.hip.h
    assert slots(3072) == 8192 and slots(3073) == 16384 and slots(257) == 4096


# ---- host: the vectorised references ---------------------------------------------------------------------------------------------
def ranking_input(m, kind):
    rng = np.random.default_rng(m)
    if kind == "plain":
        s = rng.standard_normal(m).astype(np.float32).astype(np.float64)
    else:
        s = tied_scores(rng, m)
        if kind == "mixed":  # heavy ties, the special values, and a fourth of the positions a group of their own
            s[::4] = rng.standard_normal(len(s[::4]))
    y = (rng.random(m) < 0.4).astype(np.uint8)
    y[0], y[1] = 1, 0
    return s, y


@pytest.mark.parametrize("m", [2, 1023, 1025, 5000])
@pytest.mark.parametrize("kind", ["ties", "plain", "mixed"])
def test_vectorised_ranking_equals_the_restatement(m, kind):
    s, y = ranking_input(m, kind)
    got, want = S.ranking(s, y), HR.ranking(s, y)
    assert got.keys() == want.keys()
    for k in ("concordant", "tied", "positives", "negatives", "groups"):
        assert got[k] == want[k] and isinstance(got[k], int), k
    assert np.float64(got["auc"]).tobytes() == np.float64(want["auc"]).tobytes() and np.float64(got["ap"]).tobytes() == np.float64(want["ap"]).tobytes()
    assert [int(k) for k in S.order_keys(s)] == [HR.order_key(x) for x in s]


def test_blocked_sum_is_the_running_sum_of_the_definition():
    terms = np.random.default_rng(1).random(3000) * np.array([1e-8, 1.0, 1e8])[np.arange(3000) % 3]
    total = 0.0
    for b in range(0, 3000, 1024):
        block = 0.0
        for t in terms[b:b + 1024]:
            block += float(t)
        total += block
    assert S.blocked_sum(terms) == total != S.blocked_sum(terms, 3000)  # (one running sum over all the terms rounds differently)


@pytest.mark.parametrize("name", CC_GRAPHS)
def test_vectorised_components_equal_the_restatement(name):
    got, want = S.components_fast(*cc_graph(name)), cc_comps(name)
    assert got.keys() == want.keys()
    for k in ("labels", "sizes"):
        assert got[k].dtype == want[k].dtype == np.uint32 and np.array_equal(got[k], want[k])
    assert {k: got[k] for k in CR.COMPONENT_COUNTERS} == {k: want[k] for k in CR.COMPONENT_COUNTERS}


# ---- GPU: link pairs -------------------------------------------------------------------------------------------------------------
LINK_CASES = [("thresholds", 1), ("thresholds", 2), ("medium", 1), ("large", 1)]


@gpu
@pytest.mark.parametrize("name,ratio", LINK_CASES)
def test_link_pairs_equal_the_restatement(name, ratio):
    want = S.pair_set(name, ratio)
    eng = F.Engine(*S.graph(name), 4)
    try:
        for _ in range(2):  # the second call reuses the workspaces and the tables
            got = eng.link_pairs(ratio=ratio, seed=1, details=True)
            assert same_pairs(got, want), (name, ratio, got[3], want[3])
    finally:
        eng.close()


@gpu
def test_link_short_max_on_the_boundaries_changes_nothing():
    want = S.pair_set("thresholds", 1)
    eng = F.Engine(*S.thresholds(), 4)
    try:
        assert eng.get_param("link_short_max") == 256  # the default that TOTALS stands around
        for value in (0, 64, 255, 256, 257, 1024):
            eng.set_param("link_short_max", value)
            got = eng.link_pairs(ratio=1, seed=1, details=True)
            assert same_pairs(got, want), (value, got[3], want[3])
    finally:
        eng.close()


# ---- GPU: the two splits ---------------------------------------------------------------------------------------------------------
SPLIT_CASES = [("thresholds", 0.5, 16), ("thresholds", 0.3, 1), ("medium", 0.3, 1), ("large", 0.3, 1)]


@gpu
@pytest.mark.parametrize("name,frac,ratio", SPLIT_CASES)
@pytest.mark.parametrize("keep", ["anchor", "forest"])
def test_splits_equal_the_restatement(name, frac, ratio, keep):
    want = S.split(name, frac, ratio) if keep == "anchor" else S.split_connected(name, frac, ratio)
    assert want["held"] > 0 and want["negatives"] > 0
    eng = F.Engine(*S.graph(name), 4)
    try:
        for _ in range(2):
            got = eng.edge_split(frac=frac, seed=1, ratio=ratio, details=True, keep=keep)
            assert same_split(got, want), (name, frac, ratio, keep, got.info, {k: want[k] for k in HR.SPLIT_COUNTERS})
    finally:
        eng.close()


# ---- GPU: components, forests, subgraphs ---------------------------------------------------------------------------------------------
def same_components(got, want):
    labels, info = got
    return labels.dtype == info.sizes.dtype == np.uint32 and np.array_equal(labels, want["labels"]) and np.array_equal(info.sizes, want["sizes"]) and \
        {k: getattr(info, k) for k in CR.COMPONENT_COUNTERS} == {k: want[k] for k in CR.COMPONENT_COUNTERS}


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_components_equal_the_restatement(name):
    want = S.components(name)
    eng = F.Engine(*S.graph(name), 4)
    try:
        for _ in range(2):
            got = eng.components(details=True)
            assert same_components(got, want), (name, got[1], {k: want[k] for k in CR.COMPONENT_COUNTERS})
    finally:
        eng.close()


@gpu
def test_components_past_the_cap_of_the_thread_grids():
    """n = 16384 * 256 + 1000: cc_iota, cc_jump, cc_size and cc_stat stride"""
    rowptr, colids = S.huge()
    want = S.components_fast(rowptr, colids)
    eng = F.Engine(rowptr, colids, 4)
    try:
        for _ in range(2):
            got = eng.components(details=True)
            assert same_components(got, want), (got[1], {k: want[k] for k in CR.COMPONENT_COUNTERS})
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_forests_equal_the_restatement(name):
    c = S.components(name)
    eng = F.Engine(*S.graph(name), 4)
    try:
        for bits in (64, 1) if name == "thresholds" else (64,):
            eng.set_param("forest_key_bits", bits)
            for greatest in (False, True):
                wu, wv = S.forest(name, greatest, bits)
                for _ in range(2):
                    u, v, info = eng.spanning_forest(seed=1, greatest=greatest, details=True)
                    assert u.dtype == v.dtype == np.uint32 and np.array_equal(u, wu) and np.array_equal(v, wv), (name, bits, greatest)
                    assert len(u) == len(c["labels"]) - c["components"] == info.forest_edges and (info.components, info.edges) == (c["components"], c["edges"])
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_subgraphs_equal_the_restatement(name):
    eng = F.Engine(*S.graph(name), 4)
    try:
        for which, keep in S.keep_masks(name).items():
            want = S.subgraph(name, which)
            assert 0 < len(want[2]) == int(keep.sum())  # (`thresholds` is one component: its largest keeps every vertex)
            for _ in range(2):
                assert same_subgraph(eng.subgraph(keep), want), (name, which)
        assert same_subgraph(eng.largest_component(), S.subgraph(name, "largest"))
    finally:
        eng.close()


# ---- GPU: communities, their agreement and modularity ------------------------------------------------------------------------------
LOUVAIN_CASES = {"thresholds": (32, 64), "medium": (2, 3), "large": (2, 3)}  # (max_levels, max_sweeps): `thresholds` runs to the end


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_communities_equal_the_restatement(name):
    levels, sweeps = LOUVAIN_CASES[name]
    want = S.louvain(name, levels, sweeps)
    eng = F.Engine(*S.graph(name), 4)
    try:
        for _ in range(2):
            same_communities(eng.communities(seed=1, max_levels=levels, max_sweeps=sweeps, details=True), want, (name, "default"))
        if name == "thresholds":
            assert want["records"][-1]["qnum"] == want["records"][-1]["start"]  # run to the end: the last level merges nothing
            for short_max, slots in ((256, 0), (0, 0)):  # rows up to 256 by 16 lanes, 257 and up in the workspace | every table in the workspace
                eng.set_param("louvain_short_max", short_max)
                eng.set_param("louvain_lds_slots", slots)
                same_communities(eng.communities(seed=1, details=True), want, (name, short_max, slots))
    finally:
        eng.close()


@gpu
def test_agreement_and_modularity_of_the_communities_of_large():
    rowptr, colids = S.large()
    n = len(rowptr) - 1
    want = S.louvain("large", 2, 3)
    labels, other = want["labels"], (np.arange(n) % 1000).astype(np.uint32)
    ka, kb = want["communities"], 1000
    agree = VR.agreement(labels, ka, other, kb)
    edges, inside, degree = KR.tallies(rowptr, colids, labels, ka)
    eng = F.Engine(rowptr, colids, 4)
    try:
        for _ in range(2):
            got = eng.agreement(labels.astype(np.int64), other.astype(np.int64))
            for key in INTEGERS + FLOATS:
                assert getattr(got, key) == agree[key], (key, getattr(got, key), agree[key])
            q = eng.modularity(labels, ka)
            assert q.edges == edges == want["edges"] and np.array_equal(q.inside, inside) and np.array_equal(q.degree, degree)
            assert q.q == KR.modularity_q(edges, inside, degree) and int(q.degree.sum()) == 2 * q.edges
    finally:
        eng.close()


# ---- GPU: ranking and pair scores ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare():
    eng = F.Engine(*csr(N_ROWS, []), 4)
    yield eng
    eng.close()


@gpu
@pytest.mark.parametrize("m", RANK_SIZES)
def test_ranking_equals_the_vectorised_reference_under_a_permutation(bare, m):
    for kind in ("mixed",) if m > 2 ** 20 else ("ties", "mixed"):
        s, y = ranking_input(m, kind)
        assert np.isnan(s).any() and np.isinf(s).any() and (np.signbit(s) & (s == 0)).any()
        want = S.ranking(s, y)
        got = bare.ranking(s, y)
        assert same_ranking(got, want), (m, kind, got, want)
        assert tuple(bare.ranking(s, y))[:-1] == tuple(got)[:-1], (m, kind)  # again on the same workspaces
        p = np.random.default_rng(7).permutation(m)
        assert tuple(bare.ranking(s[p], y[p]))[:-1] == tuple(got)[:-1], (m, kind)  # a shuffled input: identical bits


@gpu
@pytest.mark.parametrize("D", [4, 100])
def test_pair_scores_past_the_cap_of_65536_wavefronts(D):
    X = matrix(D)
    u, v = pairs(PAIRS_M)
    every = np.arange(N_ROWS * N_ROWS, dtype=np.int64)
    at = u.astype(np.int64) * N_ROWS + v.astype(np.int64)
    assert len(u) == PAIRS_M and len(np.unique(at)) == N_ROWS * N_ROWS and np.isinf(X).any(axis=1).sum() == 1 and np.isnan(X).any(axis=1).sum() == 1
    eng = F.Engine(*csr(N_ROWS, []), D)
    try:
        eng.set_embeddings(X)
        for metric in ("dot", "l2", "cos"):
            want = HR.pair_scores(X, every // N_ROWS, every % N_ROWS, metric)[at]  # the restatement is a function of the pair alone
            eng.set_param("pairs_chunk", 1 << 23)  # one launch of all the pairs
            one = eng.pair_scores(u, v, metric)
            eng.set_param("pairs_chunk", 1 << 20)  # five launches
            got = eng.pair_scores(u, v, metric)
            assert got.dtype == np.float32 and got.tobytes() == one.tobytes(), (D, metric)
            assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want) & ~np.isnan(want)), (D, metric)
    finally:
        eng.close()
