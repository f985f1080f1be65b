"""Nearest-neighbour queries over the embedding matrix (include/f2v.h: f2v_nearest_rows, f2v_nearest_vectors,
f2v_neighbour_recall; Engine.nearest / neighbour_recall; the CLI's -nearest).

Host tests (no GPU): argument checks, the CLI's refusals before the graph is read, and the compiled gfx950 code of the dot kernel
(an fp32-input MFMA in its innermost loop, no scratch, nothing spilled).  -m gpu: ids and scores bit for bit against the numpy
restatement of the definition (tests/nearest_ref.py), an fp64 check that does not share it, the tie rule and padding, the
exclusions, independence of query grouping / tunables / handle, the vectors form, non-interference with training, the recall
count and the CLI's .nn file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import nearest_ref as R
from test_gather_isa import FLAGS, HIPCC, function, metadata

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu
METRICS = ("dot", "l2", "cos")
MID = {"dot": _lib.SIM_DOT, "l2": _lib.SIM_L2, "cos": _lib.SIM_COSINE}


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_nearest_entry_points_reject_null_arguments():
    L = _lib.lib()
    ids = np.zeros(4, dtype=np.uint32)
    out = np.zeros(40, dtype=np.uint32)
    u32, f32 = _lib.u32p, _lib.f32p
    assert L.f2v_nearest_rows(None, ids.ctypes.data_as(u32), 4, 10, 0, 0, out.ctypes.data_as(u32), None, None) == _lib.F2V_EINVAL
    assert L.f2v_nearest_vectors(None, None, 4, 10, 0, out.ctypes.data_as(u32), None, None) == _lib.F2V_EINVAL
    assert L.f2v_neighbour_recall(None, None, 0, 10, 0, None, None, None) == _lib.F2V_EINVAL
    assert F.NEAREST_MAX_K == 128 and (F.SIM_DOT, F.SIM_L2, F.SIM_COSINE) == (0, 1, 2)
    assert (F.NEAREST_EXCLUDE_SELF, F.NEAREST_EXCLUDE_NEIGHBOURS) == (1, 2)


@pytest.mark.parametrize("args,word", [(["-nearest", "-1"], "-nearest"), (["-nearest", "129"], "-nearest"),
                                       (["-nearest", "5", "-metric", "foo"], "-metric"), (["-nearest", "5", "-gpus", "2"], "-nearest")])
def test_cli_rejects_bad_nearest_before_reading_the_graph(tmp_path, args, word):
    for mtx in (os.path.join(tmp_path, "missing.mtx"), golden_graph_path("karate.mtx")):
        r = subprocess.run([CLI, "-input", mtx, "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1, r.stdout + r.stderr
        assert word in r.stdout and "Reading input" not in r.stdout, r.stdout
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


DOT128 = "nearest_kernelILb0ELi2ELi2ELi2EE"  # nearest_kernel<false, 2, 2, 2>: dot / cosine, 128 queries per workgroup (D <= 128)
FORMS = [DOT128, "nearest_kernelILb0ELi1ELi1ELi1EE", "nearest_kernelILb1ELi2ELi2ELi2EE", "nearest_kernelILb1ELi1ELi1ELi1EE"]  # all that are launched
TU = """#include "f2v_nearest.hip.h"
template __global__ void f2v::nearest_kernel<false, 2, 2, 2>(const f2v::NnArgs);
template __global__ void f2v::nearest_kernel<false, 1, 1, 1>(const f2v::NnArgs);
template __global__ void f2v::nearest_kernel<true, 2, 2, 2>(const f2v::NnArgs);
template __global__ void f2v::nearest_kernel<true, 1, 1, 1>(const f2v::NnArgs);
"""


def spills(text, symbol):
    """-> the kernel's spill and scratch figures from its metadata (SGPR spills go to VGPR lanes, not memory: still spills)."""
    for entry in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):]):
        if re.search(r"\.name:\s+%s\s*\n" % re.escape(symbol), entry):
            return {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry)}
    raise AssertionError("no metadata for " + symbol)


def innermost_loops(body):
    """-> {header: lines of all its blocks} for every innermost loop, from the compiler's loop comments.  (A rotated loop's
    body may be laid out in front of its header, so blocks are collected by their `in Loop: Header=` note, not by position.)"""
    blocks, cur = [], None
    for line in body.splitlines():
        m = re.match(r"^(\.LBB(\d+_\d+)|; %bb\.\d+):(.*)$", line)
        if m:
            cur = {"name": "BB" + m.group(2) if m.group(2) else None, "note": m.group(3), "lines": []}
            blocks.append(cur)
        elif cur is not None:
            if not cur["lines"] and "This Inner Loop Header" in line:
                cur["note"] += line
            cur["lines"].append(line)
    heads = [b["name"] for b in blocks if b["name"] and "Inner Loop Header" in b["note"]]
    return {h: sum((b["lines"] for b in blocks if b["name"] == h or ("Header=%s " % h) in b["note"] + " "), []) for h in heads}


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_dot_kernel_runs_on_the_matrix_cores(tmp_path, build):
    src, out = str(tmp_path / "nearest_isa.hip"), str(tmp_path / "nearest_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    symbol, body = function(text, DOT128)
    assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
    mfma = re.compile(r"\bv_mfma_f32_(32x32x2|16x16x4)_f32\b")
    loops = {h: l for h, l in innermost_loops(body).items() if any(mfma.search(x) for x in l)}
    assert loops, "no innermost loop of %s holds an fp32-input MFMA" % symbol
    assert max(sum(1 for x in l if mfma.search(x)) for l in loops.values()) >= 64  # one chunk of 32 dimensions, 2 x 2 tiles
    for form in FORMS:  # no instantiation uses scratch or spills anything, scalar registers included
        sym, code = function(text, form)
        assert spills(text, sym) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (sym, spills(text, sym))
        assert not re.search(r"\bscratch_(load|store)", code) and metadata(text, sym)["vgpr_count"] <= 512


def test_fma_restatement_against_libm():
    fmaf = C.CDLL("libm.so.6").fmaf
    fmaf.restype, fmaf.argtypes = C.c_float, [C.c_float] * 3
    rng = np.random.default_rng(3)
    a = rng.standard_normal(20000).astype(np.float32)
    b = rng.standard_normal(20000).astype(np.float32)
    c = (-(a.astype(np.float64) * b).astype(np.float32) * (1 + rng.integers(-2, 3, 20000) * np.float32(2 ** -23))).astype(np.float32)  # near ties
    c[::3] = rng.standard_normal(len(c[::3])).astype(np.float32)
    want = np.array([fmaf(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(R.fma32(a, b, c).view(np.uint32), want.view(np.uint32))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def load_graph(name):
    return F.read_mtx(golden_graph_path(name + ".mtx"))


def rows(eng, ids, k, metric, flags=0, scores=True):
    """f2v_nearest_rows through the C ABI -> (ids, scores)."""
    q = np.ascontiguousarray(ids, dtype=np.uint32)
    oi, os_ = np.empty((len(q), k), dtype=np.uint32), np.empty((len(q), k), dtype=np.float32)
    eng._ck(eng._L.f2v_nearest_rows(eng._h, q.ctypes.data_as(_lib.u32p), len(q), k, MID[metric], flags, oi.ctypes.data_as(_lib.u32p),
                                    os_.ctypes.data_as(_lib.f32p) if scores else None, None))
    return oi, os_


def trained(graph, option, dim, iters=100, batch=256):
    rowptr, colids = load_graph(graph)
    eng = F.Engine(rowptr, colids, dim)
    eng.srand(1)
    eng.init_embeddings(0 if option == 5 else 1)
    eng.train(option, iters, batch, 5, 0.02)
    return eng, rowptr, colids


EXACT = [  # graph, option, dim, batch
    ("cora", 5, 128, 256), ("cora", 6, 128, 256), ("karate", 5, 16, 16), ("cora", 5, 100, 256), ("cora", 6, 200, 256),
]


@gpu
@pytest.mark.parametrize("graph,option,dim,batch", EXACT, ids=["%s-o%d-D%d" % c[:3] for c in EXACT])
def test_results_equal_the_restatement_bit_for_bit(graph, option, dim, batch):
    eng, rowptr, colids = trained(graph, option, dim, batch=batch)
    try:
        X = eng.get_embeddings()
        n = X.shape[0]
        q = np.arange(n, dtype=np.uint32) if graph == "karate" else np.sort(np.random.default_rng(11).choice(n, 256, replace=False)).astype(np.uint32)
        for metric in METRICS:
            S = R.scores(X[q], X, metric)
            for flags in (0, 1, 2, 3):
                mask = R.exclusion_mask(q, n, rowptr, colids, flags & 1, flags & 2) if flags else None
                for k in (1, 10, 128):
                    got = rows(eng, q, k, metric, flags)
                    want = R.top_k(S, k, mask)
                    assert R.same(got, want), (metric, flags, k, np.argwhere(got[0] != want[0])[:4], np.argwhere(got[1] != want[1])[:4])
        assert np.array_equal(rows(eng, q, 10, "dot", 1, scores=False)[0], R.top_k(R.scores(X[q], X, "dot"), 10, R.exclusion_mask(q, n, rowptr, colids, 1, 0))[0])
    finally:
        eng.close()


def gamma(m):
    return m * R.U / (1 - m * R.U)


@gpu
@pytest.mark.parametrize("option", [5, 6])
def test_results_against_fp64(option):
    """Does not share the restatement.  B is the standard worst-case bound of the fp32 score against its exact value (Higham,
    Accuracy and Stability, section 3.1: a chain of m roundings carries a factor within 1 +- gamma_m):
      dot     D roundings of the chain: B = gamma_D sum|q_d c_d|;
      cosine  the chain, the two norms through their square roots (gamma_D / 2 each), square root and division of each norm,
              two multiplications: B = (2 gamma_D + 5u) sum|q_d c_d| r_q r_c;
      L2      every term (q_d - c_d)^2 is non-negative and carries the subtraction's rounding twice plus at most D chain
              roundings: B = gamma_(D+2) |s|.
    A returned fp32 score is within its pair's B of the fp64 score.  And a returned id j cannot lie far below the true rank-k
    candidate t: the k candidates of the fp64 top-k each have an fp32 score >= f64(t) - Bk (Bk: the largest B among them), j's
    is <= f64(j) + B_j; if f64(j) < f64(t) - Bk - B_j all k of them would precede j.  So f64(j) >= f64(t) - (B_j + Bk), the
    '2B' of the requirement with each B taken where it applies.  No set equality with the fp64 top-k is asserted: candidates
    around rank k closer than their bounds may legitimately swap."""
    eng, rowptr, colids = trained("cora", option, 128)
    try:
        X = eng.get_embeddings()
        n, D = X.shape
        X64 = X.astype(np.float64)
        q = np.arange(n, dtype=np.uint32)
        absdot = np.abs(X64) @ np.abs(X64).T
        r = 1.0 / np.sqrt((X64 * X64).sum(1))
        for metric in METRICS:
            if metric == "dot":
                S = X64 @ X64.T
                B = gamma(D) * absdot
            elif metric == "cos":
                S = (X64 @ X64.T) * r[:, None] * r[None, :]
                B = (2 * gamma(D) + 5 * R.U) * absdot * r[:, None] * r[None, :]
            else:
                S = -((X64 * X64).sum(1)[:, None] + (X64 * X64).sum(1)[None, :] - 2 * (X64 @ X64.T))
                for lo in range(0, n, 64):  # from differences, in fp64 (the expansion above only sizes the array)
                    S[lo:lo + 64] = -((X64[lo:lo + 64, None, :] - X64[None, :, :]) ** 2).sum(2)
                B = gamma(D + 2) * np.abs(S)
            for k in (10, 100):
                ids, sc = rows(eng, q, k, metric, 0)
                assert np.all(ids != R.PAD_ID)
                idx = ids.astype(np.int64)
                s64 = np.take_along_axis(S, idx, 1)
                b = np.take_along_axis(B, idx, 1)
                worst = np.max(np.abs(sc.astype(np.float64) - s64) - b)
                print("fp64 check option %d %s k=%d: max(|s32 - s64| - B) = %.3g" % (option, metric, k, worst))
                assert np.all(np.abs(sc.astype(np.float64) - s64) <= b), (metric, k, worst)
                top = np.argsort(-S, axis=1, kind="stable")[:, :k]
                t64 = np.take_along_axis(S, top, 1)[:, -1]
                bk = np.take_along_axis(B, top, 1).max(1)
                slack = s64 - (t64[:, None] - (b + bk[:, None]))
                print("fp64 check option %d %s k=%d: min slack %.3g" % (option, metric, k, slack.min()))
                assert np.all(slack >= 0), (metric, k, slack.min())
    finally:
        eng.close()


@gpu
def test_tie_rule_padding_and_nan():
    rowptr, colids = load_graph("karate")
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 16)
    try:
        rng = np.random.default_rng(5)
        eng.set_embeddings(np.tile(rng.standard_normal(16).astype(np.float32), (n, 1)))  # all rows equal: ids ascending
        q = np.arange(n, dtype=np.uint32)
        for metric in METRICS:
            ids, sc = rows(eng, q, 10, metric, 0)
            assert np.array_equal(ids, np.tile(np.arange(10, dtype=np.uint32), (n, 1))), metric
            assert np.all(sc == sc[0, 0])
            ids, _ = rows(eng, q, 5, metric, 1)
            assert np.array_equal(ids[0], [1, 2, 3, 4, 5]) and np.array_equal(ids[3], [0, 1, 2, 4, 5])
        X = np.repeat(rng.standard_normal((9, 16)).astype(np.float32), 4, axis=0)[:n]  # rows duplicated in blocks of four
        eng.set_embeddings(X)
        for metric in METRICS:
            got = rows(eng, q, 12, metric, 0)
            assert R.same(got, R.nearest_ref(X, 12, metric, qids=q)), metric
            blocks = got[0][:, :12] // 4
            tied = (blocks[:, 1:] == blocks[:, :-1]) & (got[1][:, 1:] == got[1][:, :-1])
            assert tied.any() and np.all(got[0][:, 1:][tied] > got[0][:, :-1][tied])
        # k = 64 on 34 vertices, self excluded: 33 candidates, the tail is padding
        X = rng.standard_normal((n, 16)).astype(np.float32)
        X[7] = np.nan  # a row of NaNs: every score with it is NaN and ranks last
        eng.set_embeddings(X)
        for metric in METRICS:
            ids, sc = rows(eng, q, 64, metric, 1)
            assert np.all(ids[:, 33:] == R.PAD_ID) and np.all(np.isneginf(sc[:, 33:]))
            assert np.all(ids[:, :33] != R.PAD_ID)
            others = np.delete(q, 7)
            assert np.all(ids[others, 32] == 7) and np.all(np.isnan(sc[others, 32])) and not np.isnan(sc[others, :32]).any()
            assert np.array_equal(ids[7, :33], others) and np.all(np.isnan(sc[7, :33]))  # NaNs among themselves: ascending id
            assert R.same((ids, sc), R.nearest_ref(X, 64, metric, qids=q, rowptr=rowptr, colids=colids, exclude_self=True)), metric
    finally:
        eng.close()


@gpu
def test_exclusions():
    eng, rowptr, colids = trained("cora", 5, 128, iters=20)
    try:
        X = eng.get_embeddings()
        deg = np.diff(rowptr.astype(np.int64))
        hub = int(np.argmax(deg))
        q = np.array([hub, int(np.argmin(deg)), 5, 2000], dtype=np.uint32)
        for metric in METRICS:
            for flags in (2, 3):
                ids, sc = rows(eng, q, 128, metric, flags)
                for i, v in enumerate(q):
                    nb = colids[rowptr[v]:rowptr[v + 1]]
                    assert not np.isin(ids[i], nb).any(), (metric, flags, v)
                    assert flags == 2 or v not in ids[i]
                assert R.same((ids, sc), R.nearest_ref(X, 128, metric, qids=q, rowptr=rowptr, colids=colids, exclude_self=flags & 1, exclude_neighbours=True))
    finally:
        eng.close()
    rp = np.concatenate([rowptr, rowptr[-1:]]).astype(np.uint32)  # one more vertex, of degree 0
    eng = F.Engine(rp, colids, 32)
    try:
        eng.srand(2)
        eng.init_embeddings(0)
        X = eng.get_embeddings()
        q = np.array([len(rp) - 2, hub], dtype=np.uint32)
        got = rows(eng, q, 20, "l2", 3)
        assert R.same(got, R.nearest_ref(X, 20, "l2", qids=q, rowptr=rp, colids=colids, exclude_self=True, exclude_neighbours=True))
        assert R.same(rows(eng, q[:1], 20, "l2", 2), rows(eng, q[:1], 20, "l2", 0))  # no neighbours: nothing to drop
    finally:
        eng.close()


TUNABLE_EXTREMES = [  # every nearest_* tunable at both ends of its range (nearest_block = 128 exists at D <= 128 only)
    (("nearest_splits", 1), ("nearest_block", 32), ("nearest_chunk", 1)),
    (("nearest_splits", 256), ("nearest_block", 128), ("nearest_chunk", 65536)),
    (("nearest_splits", 1), ("nearest_block", 128), ("nearest_chunk", 100)),
    (("nearest_splits", 256), ("nearest_block", 32), ("nearest_chunk", 7)),
]


@gpu
def test_results_do_not_depend_on_grouping_tunables_or_handle():
    from force2vec_amd.graph import rmat_csr
    rowptr, colids = rmat_csr(16)
    n = len(rowptr) - 1

    def engine():
        eng = F.Engine(rowptr, colids, 128)
        eng.srand(1)
        eng.init_embeddings(0)
        eng.train(5, 1, 65536, 5, 0.02)
        return eng

    eng = engine()
    try:
        q = np.random.default_rng(9).choice(n, 300, replace=False).astype(np.uint32)
        base = {(m, f): rows(eng, q, 10, m, f) for m in METRICS for f in (0, 3)}
        big = lambda e: rows(e, q[:64], 128, "dot", 1)
        base[("dot", 128)] = big(eng)
        for (m, f), want in [c for c in base.items() if c[0][1] != 128]:
            one = [rows(eng, q[i:i + 1], 10, m, f) for i in range(300)]
            assert R.same((np.concatenate([o[0] for o in one]), np.concatenate([o[1] for o in one])), want), (m, f)
        for (m, f), want in base.items():
            if f == 128:
                continue
            seven = [rows(eng, q[i:i + 7], 10, m, f) for i in range(0, 300, 7)]
            assert R.same((np.concatenate([o[0] for o in seven]), np.concatenate([o[1] for o in seven])), want), (m, f)
        for params in TUNABLE_EXTREMES:
            for name, v in params:
                eng.set_param(name, v)
                assert eng.get_param(name) == v
            for (m, f), want in base.items():
                got = big(eng) if f == 128 else rows(eng, q, 10, m, f)
                assert R.same(got, want), (params, m, f)
        for name in ("nearest_splits", "nearest_block"):
            eng.set_param(name, 0)
        eng.set_param("nearest_chunk", 8192)
        other = engine()
        try:
            for (m, f), want in base.items():
                got = big(other) if f == 128 else rows(other, q, 10, m, f)
                assert R.same(got, want), ("second handle", m, f)
        finally:
            other.close()
        X = eng.get_embeddings()
        for m in METRICS:  # 64 of the queries against the restatement: several candidate splits and query blocks really occurred
            want = R.nearest_ref(X, 10, m, qids=q[:64], rowptr=rowptr, colids=colids, exclude_self=True, exclude_neighbours=True)
            assert R.same((base[(m, 3)][0][:64], base[(m, 3)][1][:64]), want), m
    finally:
        eng.close()


@gpu
def test_vectors_form():
    eng, rowptr, colids = trained("cora", 6, 100, iters=10)
    try:
        X = eng.get_embeddings()
        q = np.array([0, 1, 77, 2707, 1500], dtype=np.uint32)
        stranger = np.random.default_rng(1).standard_normal((3, 100)).astype(np.float32)  # no rows of the matrix
        for metric in METRICS:
            assert R.same(eng.nearest(vectors=X[q], k=10, metric=metric), rows(eng, q, 10, metric, 0)), metric
            assert R.same(eng.nearest(vectors=stranger, k=10, metric=metric), R.nearest_ref(X, 10, metric, vectors=stranger)), metric
            assert R.same(eng.nearest(ids=q, k=10, metric=metric), rows(eng, q, 10, metric, 1))  # Engine.nearest: self excluded by default
            assert R.same(eng.nearest(ids=q, k=10, metric=metric, exclude_self=False, exclude_neighbours=True), rows(eng, q, 10, metric, 2))
        ids, sc = eng.nearest(k=3)
        assert ids.shape == (2708, 3) and sc.dtype == np.float32 and eng.last_nearest_seconds > 0
    finally:
        eng.close()


@gpu
def test_state_and_argument_errors():
    rowptr, colids = load_graph("cora")
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 128)
    try:
        L, h = eng._L, eng._h
        q = np.array([1, 2], dtype=np.uint32)
        oi, os_ = np.zeros((2, 10), dtype=np.uint32), np.zeros((2, 10), dtype=np.float32)
        hits, poss = C.c_uint64(), C.c_uint64()
        call = lambda k=10, metric=0, flags=0, nq=2: L.f2v_nearest_rows(h, q.ctypes.data_as(_lib.u32p), nq, k, metric, flags, oi.ctypes.data_as(_lib.u32p), os_.ctypes.data_as(_lib.f32p), None)
        assert call() == _lib.F2V_ESTATE  # before init_embeddings
        assert L.f2v_neighbour_recall(h, None, 0, 10, 0, C.byref(hits), C.byref(poss), None) == _lib.F2V_ESTATE
        eng.srand(1)
        eng.init_embeddings(0)
        assert call(k=0) == call(k=129) == call(metric=3) == call(metric=-1) == call(flags=4) == _lib.F2V_EINVAL
        assert L.f2v_nearest_rows(h, q.ctypes.data_as(_lib.u32p), 2, 10, 0, 0, None, None, None) == _lib.F2V_EINVAL
        assert L.f2v_nearest_vectors(h, None, 2, 10, 0, oi.ctypes.data_as(_lib.u32p), None, None) == _lib.F2V_EINVAL
        q[1] = n
        assert call() == _lib.F2V_EINVAL  # not a vertex
        q[1] = 2
        oi[:] = 12345
        assert call(nq=0) == _lib.F2V_OK and np.all(oi == 12345)
        assert call() == _lib.F2V_OK and np.all(oi < n)
        # a partial range pending: the query sees what get_embeddings would return
        ids = eng.draw_samples(n - 1, 5)
        eng.minibatch_step(5, 0, n // 2, ids, 5, 0.02)
        got = rows(eng, np.arange(40, dtype=np.uint32), 10, "l2", 1)
        X = eng.get_embeddings()
        assert R.same(got, R.nearest_ref(X, 10, "l2", qids=np.arange(40, dtype=np.uint32), rowptr=rowptr, colids=colids, exclude_self=True))
    finally:
        eng.close()


def _round_robin():
    eng = F.Engine(np.array([0, 1, 2, 2, 2], dtype=np.uint32), np.array([1, 0], dtype=np.uint32), 32)
    ok = eng.get_param("xcc_round_robin") == 1
    eng.close()
    return ok


TRAIN_FORMS = [  # name, batch, params, last_train_form where the dispatch probe allows in-grid waits (0 plain, 1 chained, 2 wide)
    ("plain", 2708, (("chain_batches", 0),), 0), ("chained", 384, (("chain_wide", 0),), 1), ("epochs_in_one_launch", 256, (), 2),
]


@gpu
@pytest.mark.parametrize("form,batch,params,expect", TRAIN_FORMS, ids=[c[0] for c in TRAIN_FORMS])
def test_queries_do_not_change_training(form, batch, params, expect):
    rowptr, colids = load_graph("cora")

    def run(query):
        eng = F.Engine(rowptr, colids, 128)
        try:
            for name, v in params:
                eng.set_param(name, v)
            eng.srand(1)
            eng.init_embeddings(0)
            eng.train(5, 5, batch, 5, 0.02)
            if query:
                for metric in METRICS:
                    eng.nearest(ids=np.arange(300), k=10, metric=metric, exclude_neighbours=True)
                eng.neighbour_recall(10, "cos")
            eng.train(5, 5, batch, 5, 0.02)
            return eng.get_embeddings(), eng.rand_index(1 << 30), eng.get_param("last_train_form"), eng.get_param("last_wide_epochs")
        finally:
            eng.close()

    a, b = run(False), run(True)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1:] == b[1:]
    if expect == 0 or _round_robin():
        assert b[2] == expect, (form, b[2:])
        assert (b[3] > 1) == (form == "epochs_in_one_launch"), (form, b[2:])


@gpu
def test_recall_without_queries_and_unsorted_rows():
    rowptr, colids = load_graph("karate")
    eng = F.Engine(rowptr, colids, 16)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        none = np.zeros(1, dtype=np.uint32)
        hits, poss = C.c_uint64(77), C.c_uint64(77)  # first call of the handle, no query: 0 of 0
        assert eng._L.f2v_neighbour_recall(eng._h, none.ctypes.data_as(_lib.u32p), 0, 10, 0, C.byref(hits), C.byref(poss), None) == _lib.F2V_OK
        assert (hits.value, poss.value) == (0, 0)
    finally:
        eng.close()
    shuffled = colids.copy()
    shuffled[rowptr[0]:rowptr[1]] = shuffled[rowptr[0]:rowptr[1]][::-1]  # row 0 descending: a row search would miss neighbours
    eng = F.Engine(rowptr, shuffled, 16)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        assert R.same(rows(eng, [0, 1], 5, "dot", 1), rows(eng, [0, 1], 5, "dot", 1))  # nothing searched: fine
        with pytest.raises(F.F2VError) as e:
            rows(eng, [0, 1], 5, "dot", 2)
        assert e.value.code == _lib.F2V_EINVAL and "ascending" in str(e.value)
        with pytest.raises(F.F2VError):
            eng.neighbour_recall(5, "dot")
    finally:
        eng.close()


@gpu
def test_neighbour_recall_equals_the_count_from_nearest():
    eng, rowptr, colids = trained("cora", 5, 128, iters=50)
    try:
        n = len(rowptr) - 1
        subset = np.random.default_rng(2).choice(n, 500, replace=False).astype(np.uint32)
        for metric in ("l2", "dot", "cos"):
            for k in (1, 10, 128):
                for q in (None, subset):
                    qq = np.arange(n, dtype=np.uint32) if q is None else q
                    ids, _ = rows(eng, qq, k, metric, 1)
                    assert eng.neighbour_recall(k, metric, ids=q) == R.recall_counts(ids, qq, k, rowptr, colids), (metric, k)
        hits, possible = eng.neighbour_recall(10, "l2")
        assert 0 < hits <= possible
    finally:
        eng.close()


@gpu
def test_cli_writes_the_nn_file(tmp_path):
    mtx = golden_graph_path("cora.mtx")
    outs = {}
    for nearest in (0, 10):
        d = tmp_path / ("nn%d" % nearest)
        d.mkdir()
        r = subprocess.run([CLI, "-input", mtx, "-iter", "50", "-batch", "256", "-output", str(d) + "/", "-binout", "1", "-nearest", str(nearest)],
                           capture_output=True, text=True, cwd=d, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        embd = [p for p in os.listdir(d) if p.endswith(".embd")]
        assert len(embd) == 1
        outs[nearest] = (r.stdout, d / embd[0])
    assert open(outs[0][1], "rb").read() == open(outs[10][1], "rb").read()
    assert "Nearest:" not in outs[0][0] and not os.path.exists(str(outs[0][1]) + ".nn")
    rowptr, colids = F.read_mtx(mtx)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, 128)
    try:
        eng.set_embeddings(F.read_embd_bin(str(outs[10][1]) + ".bin", n, 128))
        ids, sc = eng.nearest(k=10, metric="l2")  # option 5's own similarity is the default metric
        hits, possible = eng.neighbour_recall(10, "l2")
    finally:
        eng.close()
    lines = open(str(outs[10][1]) + ".nn").read().splitlines()
    assert len(lines) == n
    for v, line in enumerate(lines):
        f = line.split()
        assert int(f[0]) == v and len(f) == 21
        assert np.array_equal(np.array(f[1::2], dtype=np.uint32), ids[v])
        assert np.array_equal(np.array([float(x) for x in f[2::2]], dtype=np.float32), sc[v])  # %.9g round-trips fp32
    m = re.search(r"Nearest: k=10 metric=l2 (\S+) s, precision@k (\d+)/(\d+)", outs[10][0])
    assert m and float(m.group(1)) > 0 and (int(m.group(2)), int(m.group(3))) == (hits, possible), outs[10][0]
