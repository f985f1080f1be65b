"""The communities of the graph (include/f2v.h: communities; f2v_louvain, Engine.communities, the CLI's -communities) and the
agreement of two labellings (f2v_partition_agreement, Engine.agreement).

Host tests (no GPU): the Python restatement of the definition (tests/louvain_ref.py) -- rings of cliques, its modularity beside
networkx's Louvain, Qnum never falling, labels composed of the level labels, the hand graph's written-out values --, the agreement
formulas beside scikit-learn, the compiled kernels' metadata, the refusals of the entry points and of the CLI.  -m gpu: every label,
level label, level record and counter equal to the restatement with ==; max_levels and max_sweeps; the three placements of the table;
the modularity cross-check; independence of calls, handles, training and other scorers' workspaces; the asymmetric CSR; the
agreement's integers and floats; the CLI.

Graphs: karate, cora, `hand` (8 vertices: two triangles joined by an edge, a duplicated nonzero, two self-loops -- one on a triangle
vertex, one the only nonzero of its vertex -- and an isolated vertex), rings of cliques, two RMAT graphs, `star` (a hub with 3000
leaves that also belongs to a 6-clique: one row far longer than the rest), `iso70` (no edge) and `two` (one edge)."""
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
from force2vec_amd.graph import rmat_edges_n
import louvain_ref as R
from test_gather_isa import FLAGS, HIPCC, function
from test_linkpairs import both, csr
from test_logreg import spills

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu
NONE = 0xFFFFFFFF


def ring_of_cliques(cliques, size):
    und = []
    for q in range(cliques):
        base = q * size
        und += [(base + i, base + j) for i in range(size) for j in range(i + 1, size)]
        if cliques > 1:
            a, b = base + size - 1, ((q + 1) % cliques) * size
            if (min(a, b), max(a, b)) not in und:
                und.append((min(a, b), max(a, b)))
    return csr(cliques * size, both(sorted(set(und))))


def hand():
    und = [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (4, 5), (3, 5)]
    return csr(8, both(und) + [(0, 1), (2, 2), (6, 6)])  # (0, 1) twice in row 0; self-loops at 2 and 6; 6 has nothing else; 7 is isolated


HAND_DEGREES, HAND_2M = [2, 2, 5, 3, 2, 2, 2, 0], 18


def star():
    und = [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(0, v) for v in range(6, 3006)]
    return csr(3006, both(und))


def rmat(n, m):
    n, a, b = rmat_edges_n(n, m, seed=3)
    return csr(n, both([(int(x), int(y)) for x, y in zip(a, b)]))


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in ("karate", "cora"):
        return F.read_mtx(golden_graph_path(name + ".mtx"))
    if name.startswith("ring"):
        return ring_of_cliques(*[int(x) for x in name[4:].split("x")])
    return {"hand": hand, "star": star, "rmat300": lambda: rmat(300, 1500), "rmat5000": lambda: rmat(5000, 40000),
            "iso70": lambda: csr(70, []), "two": lambda: csr(2, both([(0, 1)]))}[name]()


@functools.lru_cache(maxsize=None)
def restated(name, seed=1, max_levels=32, max_sweeps=64):
    """shared, never modified"""
    return R.louvain(*graph(name), seed=seed, max_levels=max_levels, max_sweeps=max_sweeps)


def groups(labels):
    out = {}
    for v, l in enumerate(labels):
        out.setdefault(int(l), []).append(v)
    return sorted(out.values())


# ---- host: the definition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cliques,size", [(8, 6), (5, 40)])
def test_rings_of_cliques_return_the_cliques(cliques, size):
    r = restated("ring%dx%d" % (cliques, size))
    assert groups(r["labels"]) == [list(range(q * size, (q + 1) * size)) for q in range(cliques)]


def test_a_ring_of_small_cliques_keeps_every_clique_whole():
    r = restated("ring30x5")
    for q in range(30):
        assert len(set(r["labels"][q * 5:(q + 1) * 5].tolist())) == 1, q


@pytest.mark.parametrize("name", ["karate", "cora", "rmat300", "rmat5000"])
def test_restated_modularity_is_level_with_networkx(name):
    nx = pytest.importorskip("networkx")
    rowptr, colids = graph(name)
    n = len(rowptr) - 1
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((u, int(v)) for u in range(n) for v in colids[rowptr[u]:rowptr[u + 1]] if u < v)
    theirs = [nx.community.modularity(G, nx.community.louvain_communities(G, seed=s)) for s in range(5)]
    ours = R.modularity(rowptr, colids, restated(name)["labels"])
    print(name, "restatement", ours, "networkx seeds 0..4", theirs)
    assert ours >= 0.95 * min(theirs), (ours, theirs)


@pytest.mark.parametrize("name", ["karate", "cora", "hand", "ring30x5", "rmat300", "star", "iso70", "two"])
def test_levels_never_lower_qnum_and_labels_compose(name):
    r = restated(name)
    n = len(graph(name)[0]) - 1
    assert r["levels"] == len(r["records"]) >= 1 and r["level_labels"].shape == (r["levels"], n)
    previous = None
    for l, rec in enumerate(r["records"]):
        assert rec["qnum"] >= rec["start"] and 1 <= rec["sweeps"] <= 64
        if previous is not None:
            assert rec["start"] == previous["qnum"] and rec["nodes"] == previous["communities"]  # aggregation keeps Qnum
        previous = rec
        lab = r["level_labels"][l]
        assert sorted(set(lab.tolist())) == list(range(rec["communities"]))
        if l:  # a level only merges: the earlier label decides the later one
            finer = r["level_labels"][l - 1]
            assert len({(int(a), int(b)) for a, b in zip(finer, lab)}) == r["records"][l - 1]["communities"]
    assert np.array_equal(r["labels"], r["level_labels"][-1]) and r["communities"] == r["records"][-1]["communities"]
    last = r["records"][-1]
    assert last["qnum"] == last["start"] and last["moves"] == 0 or r["levels"] == 32


def test_the_hand_graph():
    rowptr, colids = graph("hand")
    assert rowptr.tolist() == [0, 3, 5, 9, 12, 14, 16, 17, 17] and colids[:3].tolist() == [1, 1, 2]
    r = restated("hand")
    assert r["degrees"] == HAND_DEGREES and r["two_m"] == HAND_2M and r["edges"] == 9
    assert groups(r["labels"]) == [[0, 1, 2], [3, 4, 5], [6], [7]]
    assert r["labels"].tolist() == [0, 0, 0, 1, 1, 1, 2, 3] and r["communities"] == 4
    # Qnum of that partition: in2 = (6 + 2) and 6 and 2 and 0, tot = 9, 7, 2, 0
    assert r["records"][-1]["qnum"] == (8 + 6 + 2) * 18 - (81 + 49 + 4)


def test_truncated_runs_stop_where_told():
    full, one_level, one_sweep = restated("cora"), restated("cora", 1, 1, 64), restated("cora", 1, 32, 1)
    assert one_level["levels"] == 1 and np.array_equal(one_level["labels"], full["level_labels"][0])
    assert all(rec["sweeps"] == 1 for rec in one_sweep["records"])


def test_an_asymmetric_csr_is_refused_by_the_restatement():
    with pytest.raises(ValueError):
        R.louvain(*csr(3, both([(0, 1)]) + [(1, 2)]))


# ---- host: the agreement ---------------------------------------------------------------------------------------------------------
def agreement_cases():
    rng = np.random.default_rng(11)
    n = 4000
    a, b = rng.integers(0, 37, n), rng.integers(0, 90, n)
    noisy = np.where(rng.random(n) < 0.3, rng.integers(0, 37, n), a)
    holes_a, holes_b = np.where(rng.random(n) < 0.1, -1, a), np.where(rng.random(n) < 0.2, -1, noisy)
    return {"random": (a, 37, b, 90), "related": (a, 37, noisy, 37), "identical": (a, 37, a.copy(), 37),
            "one_cluster_each": (np.zeros(n, dtype=np.int64), 1, np.zeros(n, dtype=np.int64), 1), "unlabelled": (holes_a, 37, holes_b, 37),
            "wide": (rng.integers(0, 100, n), 100, rng.integers(0, 100, n), 100)}  # 10^4 cells


@pytest.mark.parametrize("case", ["random", "related", "identical", "one_cluster_each", "unlabelled", "wide"])
def test_restated_agreement_equals_scikit_learn(case):
    metrics = pytest.importorskip("sklearn.metrics")
    a, ka, b, kb = agreement_cases()[case]
    both_ = (a >= 0) & (b >= 0)
    got = R.agreement(np.where(a < 0, NONE, a), ka, np.where(b < 0, NONE, b), kb)
    nmi, ari = metrics.normalized_mutual_info_score(a[both_], b[both_]), metrics.adjusted_rand_score(a[both_], b[both_])
    print(case, got["nmi"], nmi, got["ari"], ari)
    assert got["n"] == int(both_.sum())
    assert abs(got["nmi"] - nmi) <= 1e-9 and abs(got["ari"] - ari) <= 1e-9
    if case in ("identical", "one_cluster_each"):
        assert abs(got["nmi"] - 1.0) <= 1e-9 and abs(got["ari"] - 1.0) <= 1e-9


# N at which flog(N) - fl(N * flog(N)) / N is not 0 in fp64 (6, 22, 23, 26, 27, 39, 42, 43 among them): a single class has no entropy
# whatever that difference rounds to
ONE_CLASS_N = list(range(2, 600)) + [4000, 5999]


def test_one_cluster_each_is_one_at_every_n():
    metrics = pytest.importorskip("sklearn.metrics")
    rounded = 0
    for n in ONE_CLASS_N:
        zeros = np.zeros(n, dtype=np.int64)
        got = R.agreement(zeros, 1, zeros, 1)
        assert (got["nmi"], got["ari"], got["mi"], got["entropy_a"], got["entropy_b"], got["rows"], got["cols"], got["n"]) == (1.0, 1.0, 0.0, 0.0, 0.0, 1, 1, n), n
        assert not np.signbit(got["nmi"]) and not np.signbit(got["mi"]), n
        logn = R._log(n)
        rounded += logn - (float(n) * logn) / float(n) != 0.0
    assert rounded > 50  # the sweep does hold the values of n at which the rounded difference would have decided otherwise
    for n in (6, 22, 23, 26, 27, 39, 42, 43):
        zeros = np.zeros(n, dtype=np.int64)
        assert metrics.normalized_mutual_info_score(zeros, zeros) == 1.0 and metrics.adjusted_rand_score(zeros, zeros) == 1.0


@pytest.mark.parametrize("n", [6, 22, 23, 43, 600])
def test_one_cluster_against_several_shares_nothing(n):
    metrics = pytest.importorskip("sklearn.metrics")
    zeros, three = np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64) % 3
    for a, ka, b, kb in ((zeros, 1, three, 3), (three, 3, zeros, 1)):
        got = R.agreement(a, ka, b, kb)
        assert (got["nmi"], got["mi"]) == (0.0, 0.0) and not np.signbit(got["nmi"]), n
        assert abs(got["nmi"] - metrics.normalized_mutual_info_score(a, b)) <= 1e-9 and abs(got["ari"] - metrics.adjusted_rand_score(a, b)) <= 1e-9


# ---- host: compiled code, arguments ------------------------------------------------------------------------------------------------
GATHERS = [(form, agg) for form in (0, 1, 2) for agg in ("false", "true")]
KERNELS = ["louvain_symmetry_kernel", "louvain_degree_kernel", "louvain_init_kernel", "louvain_bin_kernelILb0EE", "louvain_bin_kernelILb1EE",
           "louvain_apply_kernel", "louvain_qnum_kernel", "louvain_qnum_wide_kernel", "louvain_flag_kernel", "louvain_scan_tile_kernel", "louvain_scan_top_kernel",
           "louvain_scan_apply_kernel", "louvain_member_count_kernel", "louvain_member_fill_kernel", "louvain_relabel_kernel", "louvain_iota_kernel",
           "agree_count_kernel", "agree_piece_kernel", "agree_log_kernel"] + \
          ["louvain_gather_kernelILi%dELb%dEE" % (form, agg == "true") for form, agg in GATHERS]
TU = '#include "f2v_louvain.hip.h"\n' + "".join("template __global__ void f2v::louvain_gather_kernel<%d, %s>(const f2v::LouvainArgs);\n" % g for g in GATHERS) + \
     "".join("template __global__ void f2v::louvain_bin_kernel<%s>(const f2v::LouvainArgs);\n" % w for w in ("true", "false"))


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "louvain_isa.hip"), str(tmp_path / "louvain_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


def test_entry_points_are_exported_and_reject_null_arguments():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"f2v_louvain", "f2v_partition_agreement"} <= names
    assert (C.sizeof(_lib.LouvainLevel), C.sizeof(_lib.LouvainInfo), C.sizeof(_lib.AgreementInfo)) == (32, 32, 96)
    header = open(os.path.join(ROOT, "include", "f2v.h")).read()
    assert "#define F2V_LOUVAIN_PHASES 8" in header and "#define F2V_AGREEMENT_MAX_CELLS (1u << 26)" in header
    assert (_lib.LOUVAIN_PHASES, _lib.AGREEMENT_MAX_CELLS, R.PHASES) == (8, 1 << 26, 8)
    for struct, cls in (("f2v_louvain_level_t", _lib.LouvainLevel), ("f2v_louvain_t", _lib.LouvainInfo), ("f2v_agreement_t", _lib.AgreementInfo)):
        m = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header)
        fields = re.findall(r"(double|uint64_t|int64_t|uint32_t)\s+([^;]*);", m.group(1))
        assert [n.strip() for _, group in fields for n in group.split(",")] == [n for n, _ in cls._fields_], struct
    L = _lib.lib()
    labels = np.zeros(8, dtype=np.uint32)
    lp, info, ag = labels.ctypes.data_as(_lib.u32p), _lib.LouvainInfo(), _lib.AgreementInfo()
    assert L.f2v_louvain(None, 1, 32, 64, lp, None, None, C.byref(info)) == _lib.F2V_EINVAL
    assert b"null" in L.f2v_last_error()
    assert L.f2v_partition_agreement(None, lp, 1, lp, 1, C.byref(ag)) == _lib.F2V_EINVAL
    assert b"null" in L.f2v_last_error()


def test_cli_help_lists_communities():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    for flag in ("-communities ", "-communities-levels ", "-communities-seed "):
        assert "\n" + flag in r.stdout, flag


@pytest.mark.parametrize("args,word", [(["-communities", "2"], "-communities must be"), (["-communities", "-1"], "-communities must be"),
                                       (["-communities", "1", "-communities-levels", "0"], "-communities-levels"),
                                       (["-communities", "1", "-communities-seed", "-3"], "-communities-seed"),
                                       (["-communities", "1", "-gpus", "2"], "-communities")])
def test_cli_rejects_bad_communities_flags_before_reading_the_graph(tmp_path, args, word):
    for mtx in (os.path.join(tmp_path, "missing.mtx"), golden_graph_path("karate.mtx")):
        r = subprocess.run([CLI, "-input", mtx, "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1, r.stdout + r.stderr
        assert word in r.stdout and "Reading input" not in r.stdout, r.stdout
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def check_same(got, want, tag=None):
    labels, info = got
    assert labels.dtype == np.uint32 and np.array_equal(labels, want["labels"]), tag
    assert (info.communities, info.levels, info.edges) == (want["communities"], want["levels"], want["edges"]), tag
    assert info.level_labels.shape == want["level_labels"].shape and np.array_equal(info.level_labels, want["level_labels"]), tag
    assert [tuple(r) for r in info.level_records] == [(w["nodes"], w["communities"], w["sweeps"], w["moves"], w["qnum"]) for w in want["records"]], tag


ALL = ("karate", "cora", "hand", "ring30x5", "rmat300", "rmat5000", "star", "iso70", "two")


@gpu
@pytest.mark.parametrize("name", ALL)
def test_communities_equal_the_restatement_bit_for_bit(name):
    eng = F.Engine(*graph(name), 4)
    try:
        for seed in (1, 2):
            got = eng.communities(seed=seed, details=True)
            check_same(got, restated(name, seed), (name, seed))
            q = eng.modularity(got[0], got[1].communities)
            assert (q.q, q.edges) == (got[1].modularity, got[1].edges), (name, seed)
        if name == "iso70":
            assert (got[1].levels, got[1].communities, got[1].modularity) == (1, 70, 0.0)
        if name == "hand":
            assert got[0].tolist() == [0, 0, 0, 1, 1, 1, 2, 3]
    finally:
        eng.close()


@gpu
def test_max_levels_and_max_sweeps_truncate_as_the_restatement():
    eng = F.Engine(*graph("cora"), 4)
    try:
        check_same(eng.communities(max_levels=1, details=True), restated("cora", 1, 1, 64))
        check_same(eng.communities(max_sweeps=1, details=True), restated("cora", 1, 32, 1))
        assert np.array_equal(eng.communities(), restated("cora")["labels"])
        for bad in (dict(max_levels=0), dict(max_sweeps=0)):
            with pytest.raises(F.F2VError):
                eng.communities(**bad)
    finally:
        eng.close()


# (louvain_short_max, louvain_lds_slots): every unit that fits 16 lanes, the others in the workspace | every unit a workgroup with its
# table in LDS (the star's hub needs all 8192 slots) | every unit's table in the workspace | a mixture
PLACEMENTS = [(256, 0), (0, 8192), (0, 0), (4, 64)]


@gpu
@pytest.mark.parametrize("name", ["karate", "star", "cora"])
def test_the_placement_of_the_tables_changes_no_bit(name):
    want = restated(name)
    eng = F.Engine(*graph(name), 4)
    try:
        assert (eng.get_param("louvain_short_max"), eng.get_param("louvain_lds_slots")) == (32, 4096)
        check_same(eng.communities(details=True), want, "default")
        for short_max, slots in PLACEMENTS:
            eng.set_param("louvain_short_max", short_max)
            eng.set_param("louvain_lds_slots", slots)
            check_same(eng.communities(details=True), want, (short_max, slots))
        for key, bad in (("louvain_short_max", -1), ("louvain_short_max", 257), ("louvain_lds_slots", 8193), ("louvain_lds_slots", -1)):
            with pytest.raises(F.F2VError):
                eng.set_param(key, bad)
    finally:
        eng.close()


@gpu
def test_calls_handles_and_training_do_not_change_the_result_nor_it_them():
    rowptr, colids = graph("karate")
    want = restated("karate")
    bare = F.Engine(rowptr, colids, 4)
    a, b = F.Engine(rowptr, colids, 16), F.Engine(rowptr, colids, 16)
    try:
        check_same(bare.communities(details=True), want)  # a handle whose embeddings were never initialised
        check_same(bare.communities(details=True), want)
        with pytest.raises(F.F2VError):
            bare.get_embeddings()
        for e in (a, b):
            e.srand(5)
            e.init_embeddings(0)
            e.train(5, 2, 16, 5, 0.02)
        check_same(a.communities(details=True), want)
        assert np.array_equal(a.get_embeddings(), b.get_embeddings())
        assert [a.rand_index(1000) for _ in range(8)] == [b.rand_index(1000) for _ in range(8)]
        a.train(5, 2, 16, 5, 0.02)
        b.train(5, 2, 16, 5, 0.02)
        assert np.array_equal(a.get_embeddings(), b.get_embeddings())
        check_same(b.communities(details=True), want)
    finally:
        for e in (bare, a, b):
            e.close()


def flat(result, name="result"):
    if isinstance(result, tuple):
        names = getattr(result, "_fields", range(len(result)))
        return [leaf for field, v in zip(names, result) if field != "seconds" for leaf in flat(v, "%s.%s" % (name, field))]
    if isinstance(result, list):
        return [leaf for i, v in enumerate(result) for leaf in flat(v, "%s.%d" % (name, i))]
    return [(name, result)]


def interleaved_calls(size):
    rng = np.random.default_rng(5)
    big = size == "large"
    n = len(graph("cora")[0]) - 1
    la, lb = rng.integers(0, 300 if big else 3, n), rng.integers(0, 200 if big else 2, n)
    return [("communities", lambda e: e.communities(max_levels=32 if big else 1, max_sweeps=64 if big else 1, details=True)),
            ("kmeans", lambda e: e.kmeans(40 if big else 3, max_iters=8, seed=1)),
            ("agreement", lambda e: e.agreement(la, lb)),
            ("modularity", lambda e: e.modularity(la)),
            ("link_pairs", lambda e: e.link_pairs(ratio=5 if big else 1, details=True))]


def cora_engine():
    rowptr, colids = graph("cora")
    eng = F.Engine(rowptr, colids, 8)
    eng.set_embeddings(np.random.default_rng(3).standard_normal((len(rowptr) - 1, 8)).astype(np.float32))
    return eng


@gpu
def test_interleaved_with_other_scorers_equals_fresh_handles():
    want = {}
    for size in ("small", "large"):
        for name, call in interleaved_calls(size):
            eng = cora_engine()
            try:
                want[size, name] = flat(call(eng))
            finally:
                eng.close()
    eng = cora_engine()
    try:
        for size in ("small", "large", "small"):
            for name, call in interleaved_calls(size):
                got = flat(call(eng))
                assert [p for p, _ in got] == [p for p, _ in want[size, name]]
                for (path, x), (_, y) in zip(got, want[size, name]):
                    assert np.array_equal(np.asarray(x), np.asarray(y)), (size, name, path)
    finally:
        eng.close()


@gpu
def test_an_asymmetric_csr_is_refused_and_the_handle_still_trains():
    rowptr, colids = csr(40, both([(v, v + 1) for v in range(39)]) + [(3, 9)])  # (3, 9) without (9, 3)
    eng, twin = F.Engine(rowptr, colids, 8), F.Engine(rowptr, colids, 8)
    try:
        with pytest.raises(F.F2VError) as err:
            eng.communities()
        assert err.value.code == _lib.F2V_EINVAL and "symmetric" in str(err.value)
        for e in (eng, twin):
            e.srand(3)
            e.init_embeddings(0)
            e.train(5, 2, 8, 5, 0.02)
        assert np.array_equal(eng.get_embeddings(), twin.get_embeddings())
        with pytest.raises(F.F2VError):
            eng.communities()  # the verdict is kept
    finally:
        eng.close()
        twin.close()


INTEGERS = ("n", "sum_comb", "sum_a", "sum_b", "total", "rows", "cols")
FLOATS = ("nmi", "ari", "mi", "entropy_a", "entropy_b")


def check_agreement(eng, a, b, tag):
    """== against the restatement always; to 1e-9 against scikit-learn where it is installed"""
    (la, ka), (lb, kb) = eng._labelling(a), eng._labelling(b)
    got, want = eng.agreement(a, b), R.agreement(la, ka, lb, kb)
    for key in INTEGERS + FLOATS:
        assert getattr(got, key) == want[key], (tag, key, getattr(got, key), want[key])
    try:
        from sklearn import metrics
    except ImportError:
        return got
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    keep = (a >= 0) & (b >= 0)
    nmi, ari = metrics.normalized_mutual_info_score(a[keep], b[keep]), metrics.adjusted_rand_score(a[keep], b[keep])
    print(tag, got.nmi, nmi, got.ari, ari)
    assert abs(got.nmi - nmi) <= 1e-9 and abs(got.ari - ari) <= 1e-9, tag
    return got


@gpu
def test_agreement_equals_the_restatement_and_scikit_learn():
    rowptr, colids = graph("cora")
    n = len(rowptr) - 1
    truth = np.loadtxt(golden_graph_path("cora.nodes.labels"), dtype=np.int64)
    classes = np.full(n, -1, dtype=np.int64)
    classes[truth[:, 0] - (1 if truth[:, 0].min() == 1 else 0)] = truth[:, 1]
    rng = np.random.default_rng(2)
    eng = cora_engine()
    try:
        communities = eng.communities().astype(np.int64)
        check_agreement(eng, eng.kmeans(7, max_iters=20, seed=1).labels.astype(np.int64), communities, "kmeans against louvain")
        check_agreement(eng, np.where(rng.random(n) < 0.25, -1, classes), communities, "ground truth with holes against louvain")
        for ka, kb in ((31, 33), (32, 32), (25, 41)):  # 1023, 1024 and 1025 cells: the piece boundary
            a, b = rng.integers(0, ka, n), rng.integers(0, kb, n)
            a[:ka], b[:kb] = np.arange(ka), np.arange(kb)
            check_agreement(eng, a, b, (ka, kb))
        check_agreement(eng, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), "1 x 1")
        one = eng.agreement(np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
        assert (one.nmi, one.ari, one.rows, one.cols, one.n) == (1.0, 1.0, 1, 1, n)
        for N in (6, 22, 23, 43):  # most vertices unlabelled: N at which the rounded entropy of a single class is not 0
            few, chosen = np.full(n, -1, dtype=np.int64), rng.permutation(n)[:N]
            few[chosen] = 0
            one = check_agreement(eng, few, few.copy(), ("1 x 1", N))
            assert (one.nmi, one.ari, one.mi, one.entropy_a, one.entropy_b, one.rows, one.cols, one.n) == (1.0, 1.0, 0.0, 0.0, 0.0, 1, 1, N), N
            three = np.full(n, -1, dtype=np.int64)
            three[chosen] = np.arange(N) % 3
            split = check_agreement(eng, few, three, ("1 x 3", N))
            assert (split.nmi, split.mi, split.entropy_a, split.rows, split.cols) == (0.0, 0.0, 0.0, 1, 3) and split.entropy_b > 0.0, N
    finally:
        eng.close()


@gpu
def test_agreement_refusals():
    rowptr, colids = graph("karate")
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 4)
    L = eng._L
    try:
        lab = np.zeros(n, dtype=np.uint32)
        high = lab.copy()
        high[5] = 3
        lp, hp, out = lab.ctypes.data_as(_lib.u32p), high.ctypes.data_as(_lib.u32p), _lib.AgreementInfo()
        assert L.f2v_partition_agreement(eng._h, lp, 1, lp, 1, C.byref(out)) == _lib.F2V_OK
        for args in ((None, 1, lp, 1, C.byref(out)), (lp, 1, None, 1, C.byref(out)), (lp, 1, lp, 1, None),  # null pointers
                     (lp, 0, lp, 1, C.byref(out)), (hp, 3, lp, 1, C.byref(out)), (lp, 1, hp, 3, C.byref(out)),  # a label at its bound
                     (lp, 1 << 13, lp, (1 << 13) + 1, C.byref(out))):  # over the cap
            assert L.f2v_partition_agreement(eng._h, *args) == _lib.F2V_EINVAL, args[1:4]
        assert L.f2v_partition_agreement(eng._h, lp, 1 << 13, lp, 1 << 13, C.byref(out)) == _lib.F2V_OK  # exactly the cap
        lonely = np.full(n, NONE, dtype=np.uint32)
        lonely[0] = 0
        assert L.f2v_partition_agreement(eng._h, lonely.ctypes.data_as(_lib.u32p), 1, lp, 1, C.byref(out)) == _lib.F2V_EINVAL  # N < 2
        info = _lib.LouvainInfo()
        assert L.f2v_louvain(eng._h, 1, 32, 64, None, None, None, C.byref(info)) == _lib.F2V_EINVAL
        assert L.f2v_louvain(eng._h, 1, 32, 64, lp, None, None, None) == _lib.F2V_EINVAL
        assert L.f2v_louvain(eng._h, 1, 32, 64, lp, None, None, C.byref(info)) == _lib.F2V_OK  # the optional outputs may be NULL
        assert np.array_equal(lab, restated("karate")["labels"])
    finally:
        eng.close()


@gpu
def test_cli_prints_the_agreement_with_ground_truth_labels(tmp_path):
    mtx, truth_path = golden_graph_path("cora.mtx"), golden_graph_path("cora.nodes.labels")
    r = subprocess.run([CLI, "-input", mtx, "-iter", "1", "-dim", "8", "-batch", "256", "-option", "5", "-communities", "1", "-communities-seed", "2",
                        "-separation", truth_path, "-output", str(tmp_path) + "/"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rowptr, colids = graph("cora")
    truth = np.loadtxt(truth_path, dtype=np.int64)
    classes = np.full(len(rowptr) - 1, -1, dtype=np.int64)
    classes[truth[:, 0] - 1] = truth[:, 1]
    eng = F.Engine(rowptr, colids, 4)
    try:
        labels, info = eng.communities(seed=2, details=True)
        ag = eng.agreement(classes, labels)
    finally:
        eng.close()
    m = re.search(r"Modularity: Louvain = (\S+) Communities: (\d+) Levels: (\d+)", r.stdout)
    assert m and (float(m.group(1)), int(m.group(2)), int(m.group(3))) == (info.modularity, info.communities, info.levels), r.stdout
    m = re.search(r"Agreement\(labels, louvain\): NMI (\S+) ARI (\S+)", r.stdout)
    assert m and (float(m.group(1)), float(m.group(2))) == (ag.nmi, ag.ari), r.stdout
    assert "Agreement(kmeans" not in r.stdout


@gpu
def test_cli_writes_the_com_file_and_prints_the_agreement(tmp_path):
    mtx = golden_graph_path("karate.mtx")
    r = subprocess.run([CLI, "-input", mtx, "-iter", "3", "-dim", "16", "-batch", "16", "-option", "5", "-binout", "1", "-cluster", "4", "-communities", "1",
                        "-output", str(tmp_path) + "/"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    embd = [p for p in os.listdir(tmp_path) if p.endswith(".embd")]
    assert len(embd) == 1
    rowptr, colids = F.read_mtx(mtx)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 16)
    try:
        eng.set_embeddings(F.read_embd_bin(str(tmp_path / embd[0]) + ".bin", n, 16))
        labels, info = eng.communities(details=True)
        ag = eng.agreement(eng.kmeans(4, 300, seed=1, restarts=10).labels, labels)
    finally:
        eng.close()
    lines = open(str(tmp_path / embd[0]) + ".com").read().splitlines()
    assert [int(x.split()[0]) for x in lines] == list(range(n))
    assert np.array_equal(np.array([int(x.split()[1]) for x in lines], dtype=np.uint32), labels)
    m = re.search(r"Modularity: Louvain = (\S+) Communities: (\d+) Levels: (\d+)", r.stdout)
    assert m, r.stdout
    assert (float(m.group(1)), int(m.group(2)), int(m.group(3))) == (info.modularity, info.communities, info.levels)
    m = re.search(r"Agreement\(kmeans, louvain\): NMI (\S+) ARI (\S+)", r.stdout)
    assert m, r.stdout
    assert (float(m.group(1)), float(m.group(2))) == (ag.nmi, ag.ari)
