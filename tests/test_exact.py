"""Exact all-pairs Force2Vec, option 1 (include/f2v.h: its own section; f2v_train, f2v_objective, the CLI's -option 1).

Host tests (no GPU): the two numpy restatements of tests/exact_ref.py against the goldens of the genuine reference binary
(tests/golden/exact_manifest.json) -- the reference's order reproduces each golden's text exactly, the engine's order stays within
four times the difference recorded there --, the output name, what the CLI refuses.  -m gpu: the kernels bit for bit against the
engine-order restatement, the goldens, "exact_rows", "exact_epoch", isolation from the rand() stream and the sampled options, the
objective and its log, the refusals, the CLI."""
import functools
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, golden_graph_path

import exact_ref as R
import force2vec_amd as F
from force2vec_amd import _lib
from oracle import oracle as O

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu

with open(os.path.join(GOLD, "exact_manifest.json")) as _f:
    MANIFEST = json.load(_f)
GOLDENS = [c["name"] for c in MANIFEST["cases"]]


def golden_case(name):
    return next(c for c in MANIFEST["cases"] if c["name"] == name)


def golden_text(case):
    return b"".join(gzip.open(os.path.join(GOLD, f), "rb").read() for f in case["files"])


@functools.lru_cache(maxsize=None)
def golden_matrix(name):
    lines = golden_text(golden_case(name)).decode().splitlines()
    n, d = (int(t) for t in lines[0].split())
    X = np.zeros((n, d), dtype=np.float32)
    for line in lines[1:]:
        p = line.split()
        if p:
            X[int(p[0]) - 1] = np.array(p[1:1 + d], dtype=np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in ("karate", "cora"):
        return F.read_mtx(golden_graph_path(name + ".mtx"))
    n, avg = {"one_piece": (64, 4), "spans": (1100, 6), "auto8": (2100, 3), "auto16": (4100, 3)}[name]
    rng = np.random.default_rng(n)
    rows = [np.unique(rng.integers(0, n, rng.integers(1, 2 * avg))) for _ in range(n)]
    if name == "spans":
        rows[17] = np.array([], dtype=np.int64)                     # an isolated vertex (no other row names it either: see below)
        rows = [r[r != 17] for r in rows]
        rows[40] = np.unique(np.concatenate([rows[40], [41]]))        # (start_matrix makes rows 40 and 41 equal: an edge of length 0)
        rows[40] = np.sort(np.concatenate([rows[40], rows[40][:1]]))  # a duplicated nonzero
        rows[5] = np.unique(np.concatenate([rows[5], [1030]]))        # a neighbour beyond the first span
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return rowptr, np.concatenate(rows).astype(np.uint32)


def start_matrix(name, dim):
    n = len(graph(name)[0]) - 1
    X = np.random.default_rng(1000 * dim + n).uniform(-1, 1, (n, dim)).astype(np.float32)
    if name == "spans":
        X[300] = X[1090]  # two equal rows: a = 0, the coefficient is infinite, t * d1 is NaN and scale() makes it -5
        X[41] = X[40]     # ... and two equal rows that are neighbours where the graph has the edge
    return X


# (graph, dim, batch, epochs): one partial piece; D not a power of two and a partial last minibatch; the narrowest and the widest
# row; exactly one piece; 1024 + 76 columns -- across a span, a partial last piece, a partial last minibatch of 1100 - 2 * 384 rows
# then what the defaults select beyond those: 128 < D <= 256 (a piece is staged in two halves), a minibatch of 1024 rows or more
# (the quarter-wave pair kernel), and two graphs whose single minibatch makes the automatic "exact_rows" 8 and 16
BIT_CASES = [("karate", 16, 16, 5), ("karate", 100, 7, 3), ("karate", 1, 16, 1), ("karate", 512, 16, 1), ("one_piece", 32, 48, 2),
             ("spans", 128, 384, 1), ("karate", 200, 34, 2), ("spans", 128, 1100, 1), ("auto8", 4, 2100, 1), ("auto16", 4, 4100, 1)]


def automatic_rows(n, rows):
    """The rule of "exact_rows" = 0: the most rows per workgroup (16, 8) that still leave 1024 workgroups, else 4."""
    slices = -(-n // 1024) + 1
    return next((r for r in (16, 8) if -(-rows // r) * slices >= 1024), 4)


@functools.lru_cache(maxsize=None)
def restated(name, dim, batch, epochs):
    rowptr, colids = graph(name)
    X = R.train(start_matrix(name, dim), rowptr, colids, batch, epochs, order="engine")
    X.setflags(write=False)
    return X


def trained(name, dim, batch, epochs, params=(), calls=None):
    rowptr, colids = graph(name)
    eng = F.Engine(rowptr, colids, dim)
    try:
        for k, v in params:
            eng.set_param(k, v)
        eng.set_embeddings(start_matrix(name, dim))
        for e in calls or [epochs]:
            eng.train(1, e, batch)
        info = dict(eng.stats(), form=eng.get_param("last_train_form"), epoch=eng.get_param("exact_epoch"),
                    exact_rows=eng.get_param("last_exact_rows"), quarter=eng.get_param("last_exact_quarter"))
        return eng.get_embeddings(), info
    finally:
        eng.close()


# ---- host ------------------------------------------------------------------------------------------------------------------
def test_manifest_records_the_measured_tolerances():
    assert len(MANIFEST["cases"]) == 3
    for c in MANIFEST["cases"]:
        assert 0 < c["engine_order_max_abs_diff"] < 1e-3, c["name"]  # above 1e-3 a run has started to diverge
        assert hashlib.md5(golden_text(c)).hexdigest() == c["md5"]
        assert all(os.path.getsize(os.path.join(GOLD, f)) < (1 << 20) for f in c["files"])


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_order_reproduces_the_golden_text(name, tmp_path):
    c = golden_case(name)
    rowptr, colids = O.read_mtx(golden_graph_path(c["graph"]))
    X0 = O.Rng(1).init_embeddings(len(rowptr) - 1, c["dim"], 0)  # srand(1), randInitF
    X = R.train(X0, rowptr, colids, c["batch"], c["iters"], order="reference")
    O.write_embd(str(tmp_path / "x.embd"), X)
    assert (tmp_path / "x.embd").read_bytes() == golden_text(c)


@pytest.mark.parametrize("name", GOLDENS)
def test_engine_order_is_within_the_recorded_tolerance(name):
    c = golden_case(name)
    rowptr, colids = O.read_mtx(golden_graph_path(c["graph"]))
    X0 = O.Rng(1).init_embeddings(len(rowptr) - 1, c["dim"], 0)
    X = R.train(X0, rowptr, colids, c["batch"], c["iters"], order="engine")
    err = float(np.abs(X.astype(np.float64) - golden_matrix(name)).max())
    print("%s: engine order vs golden %.3g (recorded %.3g)" % (name, err, c["engine_order_max_abs_diff"]))
    assert err <= 4 * c["engine_order_max_abs_diff"]


def test_flog_is_a_logarithm():
    x = np.concatenate([10.0 ** np.random.default_rng(3).uniform(-6, 30, 20000), [1.0, 1e-6, 1.4142135623730951, 2.0, 1.0 + 2.0 ** -52]])
    got = R.flog(x)
    assert got[-5] == 0.0
    assert np.all(np.abs(got - np.log(x)) <= 2 * np.spacing(np.abs(np.log(x))))


def test_output_name():
    assert F.output_name("/some/dir/karate.mtx", "/out/", 1, 0, 16, 16, 2, 5) == "/out/karate.mtxF2V16D16IT2.embd"
    for c in MANIFEST["cases"]:
        assert F.output_name("/x/" + c["graph"], "", 1, 0, c["batch"], c["dim"], c["iters"], 5) == c["embd_name"]
    for option in (2, 3, 4):
        with pytest.raises(_lib.F2VError):
            F.output_name("g.mtx", "", option, 0, 256, 64, 10, 5)


def test_cli_lists_option_1_and_refuses_several_gpus(tmp_path):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 1 and "1 Force2Vec (O(n^2) version" in r.stdout
    r = subprocess.run([CLI, "-input", golden_graph_path("karate.mtx"), "-option", "1", "-gpus", "2"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-option 1" in r.stdout and "-gpus" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([CLI, "-input", golden_graph_path("karate.mtx"), "-option", "1", "-bs", "1"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-option 1" in r.stdout and "-bs" in r.stdout, r.stdout + r.stderr
    for option in ("2", "3", "4"):
        r = subprocess.run([CLI, "-input", golden_graph_path("karate.mtx"), "-option", option], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "out of scope" in r.stdout


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,dim,batch,epochs", BIT_CASES)
def test_training_is_bit_exact_against_the_engine_order(name, dim, batch, epochs):
    rowptr, _ = graph(name)
    n = len(rowptr) - 1
    X, info = trained(name, dim, batch, epochs)
    want = restated(name, dim, batch, epochs)
    assert np.all(np.isfinite(want))
    bad = np.nonzero(X.view(np.uint32) != want.view(np.uint32))
    assert len(bad[0]) == 0, "%d values differ, first at %s: %r != %r" % (len(bad[0]), (bad[0][0], bad[1][0]), X[bad][0], want[bad][0])
    assert info["form"] == 0 and info["epoch"] == epochs
    assert info["rows"] == n * epochs and info["nnz"] == int(rowptr[n]) * epochs
    assert info["step_launches"] == -(-n // batch) * epochs and info["device_seconds"] > 0
    last = n - (-(-n // batch) - 1) * batch  # rows of the last minibatch: what the two "last_exact_*" answers are about
    assert info["exact_rows"] == automatic_rows(n, last)
    assert info["quarter"] == int(dim % 4 == 0 and dim <= 256 and last >= 1024)
    if name.startswith("auto"):
        assert info["exact_rows"] == int(name[4:]) and info["quarter"] == 1


# (graph, dim, batch, epochs, parameters that pin the pair kernel, quarter-wave?): NB = 1, 2 and 4 of the quarter-wave kernel, VEC =
# 1, 2, 4 and 8 of the generic one, with D not a multiple of 4 and D = 512 among them
LAYOUT_CASES = [("spans", 128, 384, 1, (("exact_quarter_min", 0),), 1), ("karate", 200, 34, 2, (("exact_quarter_min", 0),), 1),
                ("karate", 16, 16, 5, (("exact_quarter_min", 0),), 1), ("spans", 128, 384, 1, (("quarter_wave", 0),), 0),
                ("spans", 128, 1100, 1, (("quarter_wave", 0),), 0), ("karate", 100, 7, 3, (("quarter_wave", 0),), 0),
                ("karate", 200, 34, 2, (("exact_quarter_min", 1 << 20),), 0), ("karate", 1, 16, 1, (), 0), ("karate", 512, 16, 1, (), 0),
                ("auto16", 4, 4100, 1, (("quarter_wave", 0),), 0)]


@gpu
@pytest.mark.parametrize("rows", [0, 4, 8, 16])
@pytest.mark.parametrize("name,dim,batch,epochs,params,quarter", LAYOUT_CASES)
def test_exact_rows_and_the_layout_never_change_a_bit(name, dim, batch, epochs, params, quarter, rows):
    """Every instantiation of both pair kernels: "exact_rows" 4, 8, 16 are one, two, four wavefronts per workgroup of the quarter-wave
    kernel and one, two, four rows per wavefront of the generic one."""
    X, info = trained(name, dim, batch, epochs, params=params + (("exact_rows", rows),))
    assert info["quarter"] == quarter and (rows == 0 or info["exact_rows"] == rows)
    assert X.tobytes() == restated(name, dim, batch, epochs).tobytes()


@gpu
def test_exact_rows_accepts_only_its_values():
    eng = F.Engine(*graph("karate"), 16)
    try:
        with pytest.raises(F.F2VError):
            eng.set_param("exact_rows", 5)
        eng.set_param("exact_rows", 8)
        assert eng.get_param("exact_rows") == 8 and eng.get_param("exact_epoch") == 0
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_on_the_gpu(name):
    c = golden_case(name)
    rowptr, colids = F.read_mtx(golden_graph_path(c["graph"]))
    eng = F.Engine(rowptr, colids, c["dim"])
    try:
        eng.srand(1)
        eng.init_embeddings(0)  # F2V_INIT_SYMMETRIC
        eng.train(1, c["iters"], c["batch"])
        X = eng.get_embeddings()
    finally:
        eng.close()
    err = float(np.abs(X.astype(np.float64) - golden_matrix(name)).max())
    print("%s: GPU vs golden %.3g (recorded for the engine order %.3g)" % (name, err, c["engine_order_max_abs_diff"]))
    assert err <= 4 * c["engine_order_max_abs_diff"]


@gpu
def test_drop_in_class_runs_option_1(tmp_path):
    c = golden_case("karate_opt1_it5_B16_D16")
    mtx = golden_graph_path(c["graph"])
    algo = F.algorithms(F.read_mtx(mtx), mtx, str(tmp_path) + "/", dim=16)
    try:
        algo.srand(1)
        algo.AlgoForce2Vec(5, 16, 16)
        assert os.path.basename(algo.last_output) == c["embd_name"]
        assert np.abs(algo.nCoordinates.astype(np.float64) - golden_matrix(c["name"])).max() <= 4 * c["engine_order_max_abs_diff"]
    finally:
        algo.engine.close()


@gpu
def test_exact_epoch_continues_and_starts_over():
    one, i1 = trained("karate", 16, 16, 10)
    two, i2 = trained("karate", 16, 16, 10, calls=[5, 5])
    assert one.tobytes() == two.tobytes() and i1["epoch"] == i2["epoch"] == 10
    eng = F.Engine(*graph("karate"), 16)
    try:
        X0 = start_matrix("karate", 16)
        eng.set_embeddings(X0)
        eng.train(1, 3, 16)
        first = eng.get_embeddings()
        assert eng.get_param("exact_epoch") == 3
        eng.set_embeddings(X0)
        eng.train(1, 3, 16)  # epochs 3, 4, 5: smaller steps
        assert eng.get_embeddings().tobytes() != first.tobytes()
        eng.set_param("exact_epoch", 0)
        eng.set_embeddings(X0)
        eng.train(1, 3, 16)
        assert eng.get_embeddings().tobytes() == first.tobytes()
    finally:
        eng.close()


@gpu
def test_option_1_leaves_the_rand_stream_and_the_sampled_options_alone():
    rowptr, colids = graph("karate")
    X0 = start_matrix("karate", 16)
    fresh = F.Engine(rowptr, colids, 16)
    used = F.Engine(rowptr, colids, 16)
    try:
        for eng in (fresh, used):
            eng.srand(7)
            eng.set_embeddings(X0)
        draws = [fresh.rand_index(1 << 30) for _ in range(4)]
        got = [used.rand_index(1 << 30), used.rand_index(1 << 30)]
        used.train(1, 2, 16)
        got += [used.rand_index(1 << 30), used.rand_index(1 << 30)]
        assert got == draws
        fresh.train(5, 3, 16, 5, 0.02)
        used.set_embeddings(X0)
        used.train(5, 3, 16, 5, 0.02)
        assert used.get_embeddings().tobytes() == fresh.get_embeddings().tobytes()
        assert used.rand_index(1 << 30) == fresh.rand_index(1 << 30)
    finally:
        fresh.close()
        used.close()


@gpu
@pytest.mark.parametrize("name,dim", [("karate", 16), ("spans", 128)])
def test_objective_is_bit_exact_against_the_restatement(name, dim):
    rowptr, colids = graph(name)
    n = len(rowptr) - 1
    X = start_matrix(name, dim)
    want = R.objective(X, rowptr, colids)
    eng = F.Engine(rowptr, colids, dim)
    try:
        eng.set_embeddings(X)
        got = eng.objective(1)
        again = eng.objective(1, 0)  # ns is ignored
    finally:
        eng.close()
    assert got.positive_pairs == int(rowptr[n]) and got.negative_pairs == n * (n - 1)
    assert np.isfinite(want[0])
    assert np.array([got.loss, got.attraction, got.repulsion]).tobytes() == np.array(want[:3]).tobytes(), (got, want)
    assert again == got
    # ... and it is the reference's loglike: the restatement with a library's logarithm
    t = X[:, None, :].astype(np.float64) - X[None, :, :]
    r = (t * t).sum(-1)[~np.eye(n, dtype=bool)]
    assert got.repulsion == pytest.approx(-np.sum(np.log(1e-6 + r) - np.log1p(r)), rel=1e-5)


@gpu
def test_loss_log_equals_separate_calls():
    rowptr, colids = graph("karate")
    X0 = start_matrix("karate", 16)
    a = F.Engine(rowptr, colids, 16)
    b = F.Engine(rowptr, colids, 16)
    try:
        a.set_embeddings(X0)
        a.set_param("loss_every", 2)
        sec = a.train(1, 5, 16)
        ep, vals = a.train_losses()
        assert list(ep) == [2, 4, 5] and sec > 0 and a.get_param("last_loss_us") > 0
        b.set_embeddings(X0)
        for e in range(1, 6):
            b.train(1, 1, 16)
            if e in (2, 4, 5):
                o = b.objective(1)
                assert vals[list(ep).index(e)].tobytes() == np.array([o.loss, o.attraction, o.repulsion]).tobytes()
        assert a.get_embeddings().tobytes() == b.get_embeddings().tobytes()
    finally:
        a.close()
        b.close()


@gpu
def test_refusals():
    rowptr, colids = graph("karate")
    eng = F.Engine(rowptr, colids, 16)
    try:
        eng.set_embeddings(start_matrix("karate", 16))
        with pytest.raises(F.F2VError) as e:
            eng.train_sharded(1, 2, 16)
        assert e.value.code == _lib.F2V_EINVAL and "single GPU, f2v_train only" in str(e.value)
        with pytest.raises(F.F2VError) as e:
            eng.minibatch_step(1, 0, 16, np.zeros(5, dtype=np.uint32), 5, 0.02)
        assert e.value.code == _lib.F2V_EINVAL and "single GPU, f2v_train only" in str(e.value)
        eng.upload_sample_ids(np.zeros(8, dtype=np.uint32))
        with pytest.raises(F.F2VError) as e:
            eng.minibatch_step_at(1, 0, 16, 0, 5, 0.02)
        assert e.value.code == _lib.F2V_EINVAL and "single GPU, f2v_train only" in str(e.value)
        for option in (2, 3, 4):
            with pytest.raises(F.F2VError) as e:
                eng.train(option, 2, 16)
            assert e.value.code == _lib.F2V_EINVAL
            with pytest.raises(F.F2VError):
                eng.objective(option)
        with pytest.raises(F.F2VError) as e:
            eng.train(1, 2, 16, 5, 0.02, 1)
        assert e.value.code == _lib.F2V_EINVAL
        with pytest.raises(F.F2VError):
            eng.train(1, 2, 0)
        assert eng.get_param("exact_epoch") == 0
    finally:
        eng.close()


@gpu
def test_cli_runs_option_1(tmp_path):
    r = subprocess.run([CLI, "-input", golden_graph_path("karate.mtx"), "-option", "1", "-iter", "2", "-dim", "16", "-batch", "16", "-output", str(tmp_path) + "/",
                        "-loss", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Running: Force2Vec(n^2)" in r.stdout and "Force2Vec Parallel Wall time required:" in r.stdout
    out = tmp_path / "karate.mtxF2V16D16IT2.embd"
    assert out.exists() and out.read_text().splitlines()[0].split() == ["34", "16"]
    assert [l.split(":")[1].split()[0] for l in r.stdout.splitlines() if ":LOGLIKELIHOOD:" in l] == ["1", "2"]
