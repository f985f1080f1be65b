"""The training objective (include/f2v.h: f2v_objective, "loss_every", f2v_train_losses, the CLI's -loss).

Host tests (no GPU): the CLI refuses -loss with -gpus > 1 or a negative value before it reads the graph; the entry points reject
null arguments.  -m gpu: the value against a numpy restatement of the definition (hash included), determinism, non-interference
with training in every launch form, the per-epoch log, and the CLI's LOGLIKELIHOOD lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu


# ---- host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["-loss", "5", "-gpus", "2"], ["-loss", "-1"]])
def test_cli_rejects_bad_loss_before_reading_the_graph(tmp_path, args):
    r = subprocess.run([CLI, "-input", os.path.join(tmp_path, "missing.mtx"), "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "-loss" in r.stdout
    r = subprocess.run([CLI, "-input", golden_graph_path("karate.mtx"), "-iter", "3"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "-loss" in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(tmp_path, "Results.txt"))


def test_objective_entry_points_reject_null_arguments():
    L = _lib.lib()
    assert L.f2v_objective(None, 5, 5, None) == _lib.F2V_EINVAL
    assert L.f2v_train_losses(None, None, None, 0, None) == _lib.F2V_EINVAL


# ---- numpy restatement of the definition (include/f2v.h) ---------------------------------------------------------------------
def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def negative_samples(n, ns, seed=1):
    """s(i,k) = mix64(mix64(seed) ^ (i * ns + k)) % (n - 1) -> (sources, samples), row-major."""
    i = np.repeat(np.arange(n, dtype=np.uint64), ns)
    k = np.tile(np.arange(ns, dtype=np.uint64), n)
    with np.errstate(over="ignore"):
        key = i * np.uint64(ns) + k
    s = mix64(mix64(np.uint64(seed)) ^ key) % np.uint64(n - 1)
    return i.astype(np.int64), s.astype(np.int64)


def _pairwise(a, axis):
    while a.shape[axis] > 1:
        a = np.add(np.take(a, range(0, a.shape[axis], 2), axis=axis), np.take(a, range(1, a.shape[axis], 2), axis=axis))
    return np.take(a, 0, axis=axis)


def pair_scalars_kernel_order(X, a, b, sigmoid):
    """The fp32 squared distance / dot product of pairs (a, b) in the kernel's summation order: dims zero-padded to 64*VEC,
    lane t of a quarter-wave holds dims [64k + 4t, +4); (e0 + e1) + (e2 + e3), then pairwise over k, then pairwise over the 16 lanes."""
    n, D = X.shape
    vec = 1
    while 64 * vec < D:
        vec *= 2
    Xp = np.zeros((n, 64 * vec), dtype=np.float32)
    Xp[:, :D] = X
    out = np.empty(len(a), dtype=np.float32)
    step = max(1, (1 << 22) // (64 * vec))
    for lo in range(0, len(a), step):
        xa, xb = Xp[a[lo:lo + step]], Xp[b[lo:lo + step]]
        if sigmoid:
            e = xa * xb
        else:
            d = xa - xb
            e = d * d
        e = e.reshape(len(xa), vec, 16, 4)
        bs = (e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])
        out[lo:lo + step] = _pairwise(_pairwise(bs, 1), 1)
    return out


def pair_scalars_fp64(X, a, b, sigmoid):
    out = np.empty(len(a), dtype=np.float64)
    step = 1 << 15
    for lo in range(0, len(a), step):
        xa, xb = X[a[lo:lo + step]].astype(np.float64), X[b[lo:lo + step]].astype(np.float64)
        out[lo:lo + step] = (xa * xb).sum(1) if sigmoid else ((xa - xb) ** 2).sum(1)
    return out


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def objective_ref(X, rowptr, colids, option, ns, seed=1, kernel_order=True):
    n = len(rowptr) - 1
    deg = np.diff(rowptr.astype(np.int64))
    src = np.repeat(np.arange(n), deg)
    dst = colids.astype(np.int64)
    si, ss = negative_samples(n, ns, seed)
    sig = option not in (5, 8, 11)
    scal = pair_scalars_kernel_order if kernel_order else pair_scalars_fp64
    zp = scal(X, src, dst, sig).astype(np.float64)
    zn = scal(X, si, ss, sig).astype(np.float64)
    if sig:
        degi = np.ones(n) if option == 10 else 1.0 / (deg + 1.0)
        att = float(np.sum(degi[src] * softplus(-zp)))
        rep = float(np.sum(softplus(zn)))
    else:
        att = float(np.sum(np.log1p(zp)))
        rep = float(-np.sum(np.log(1e-6 + zn) - np.log1p(zn)))
    return att, rep, len(dst), n * ns


def test_negative_sample_hash_restatement():
    """The restatement's splitmix64 finaliser is the standard one (reference value of splitmix64 seeded with 0)."""
    assert int(mix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    i, s = negative_samples(10, 3)
    assert len(s) == 30 and s.min() >= 0 and s.max() < 9


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def hub_graph(n=3000, avg_deg=6, seed=7, hubs=((0, 2500), (17, 600), (2999, 300))):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n * avg_deg // 2)
    dst = rng.integers(0, n, n * avg_deg // 2)
    for h, d in hubs:
        nb = rng.choice(n, d, replace=False)
        src = np.concatenate([src, np.full(d, h)])
        dst = np.concatenate([dst, nb])
    keep = src != dst
    src, dst = src[keep], dst[keep]
    r = np.concatenate([src, dst])
    c = np.concatenate([dst, src])
    order = np.lexsort((c, r))
    rowptr = np.zeros(n + 1, dtype=np.uint32)
    rowptr[1:] = np.cumsum(np.bincount(r[order], minlength=n))
    return rowptr, c[order].astype(np.uint32)


def load_graph(name):
    if name == "hubs":
        return hub_graph()
    return F.read_mtx(golden_graph_path(name + ".mtx"))


def _bits(o):
    return (np.float64(o.loss).tobytes(), np.float64(o.attraction).tobytes(), np.float64(o.repulsion).tobytes(), o.positive_pairs, o.negative_pairs)


VALUE_CASES = [  # graph, option, dim, ns
    ("karate", 5, 16, 5), ("karate", 6, 512, 12), ("karate", 7, 100, 0), ("karate", 10, 128, 5),
    ("cora", 5, 128, 5), ("cora", 6, 100, 12), ("cora", 10, 16, 5), ("cora", 7, 512, 5), ("cora", 5, 512, 0),
    ("pubmed", 5, 100, 12), ("pubmed", 6, 128, 5), ("pubmed", 7, 16, 0),
    ("hubs", 5, 512, 5), ("hubs", 6, 16, 12), ("hubs", 10, 100, 5), ("hubs", 5, 128, 12),
]


@gpu
@pytest.mark.parametrize("graph,option,dim,ns", VALUE_CASES)
def test_objective_value(graph, option, dim, ns):
    rowptr, colids = load_graph(graph)
    eng = F.Engine(rowptr, colids, dim)
    eng.srand(1)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    try:
        for stage in ("init0", "init1", "trained"):
            if stage == "init0":
                eng.init_embeddings(0)
            elif stage == "init1":
                eng.init_embeddings(1)
            else:
                eng.train(option, 3, 256, 5, 0.02)
            X = eng.get_embeddings()
            got = eng.objective(option, ns)
            assert got.positive_pairs == nnz and got.negative_pairs == n * ns
            assert got.loss == got.attraction + got.repulsion
            att, rep, _, _ = objective_ref(X, rowptr, colids, option, ns)
            # the kernel's own fp32 pair sums restated: only the fp64 logs and the order of the fp64 sums differ
            np.testing.assert_allclose([got.attraction, got.repulsion], [att, rep], rtol=1e-10, atol=1e-300, err_msg=stage)
            # the definition in fp64 throughout: the fp32 pair sums are the difference (softplus of a large |z| amplifies it)
            att64, rep64, _, _ = objective_ref(X, rowptr, colids, option, ns, kernel_order=False)
            tol = 1e-5 if option in (5, 8, 11) else 1e-3
            np.testing.assert_allclose([got.attraction, got.repulsion], [att64, rep64], rtol=tol, atol=1e-300, err_msg=stage)
            if ns == 0:
                assert got.repulsion == 0.0
    finally:
        eng.close()


@gpu
def test_objective_state_and_argument_errors():
    rowptr, colids = load_graph("karate")
    eng = F.Engine(rowptr, colids, 16)
    try:
        with pytest.raises(F.F2VError) as e:
            eng.objective(5)
        assert e.value.code == _lib.F2V_ESTATE
        eng.init_embeddings(0)
        for bad in (4, 12):
            with pytest.raises(F.F2VError) as e:
                eng.objective(bad)
            assert e.value.code == _lib.F2V_EINVAL
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("scale", [16, 20])
def test_objective_is_deterministic(scale):
    from force2vec_amd.graph import rmat_csr
    rowptr, colids = rmat_csr(scale, 16, seed=1)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    engines = [F.Engine(rowptr, colids, 128) for _ in range(2)]
    try:
        for e in engines:
            e.srand(1)
            e.init_embeddings(0)
        for option in (5, 6):
            first = engines[0].objective(option, 5)
            assert first.positive_pairs == nnz and first.negative_pairs == 5 * n
            assert _bits(engines[0].objective(option, 5)) == _bits(first)
            assert _bits(engines[1].objective(option, 5)) == _bits(first)
        if scale == 16:
            ref = {o: _bits(engines[0].objective(o, 5)) for o in (5, 6)}
            for name, value in (("waves_per_block", 1), ("quarter_wave", 0), ("rows_in_flight", 8), ("piece_affinity", 0)):
                engines[1].set_param(name, value)
                for o in (5, 6):
                    assert _bits(engines[1].objective(o, 5)) == ref[o], name
            engines[0].set_param("loss_seed", 2)
            assert _bits(engines[0].objective(5, 5)) != ref[5]
            engines[0].set_param("loss_seed", 1)
            assert _bits(engines[0].objective(5, 5)) == ref[5]
    finally:
        for e in engines:
            e.close()


def _round_robin():
    eng = F.Engine(np.array([0, 1, 2, 2, 2], dtype=np.uint32), np.array([1, 0], dtype=np.uint32), 32)
    ok = eng.get_param("xcc_round_robin") == 1
    eng.close()
    return ok


def _run(rowptr, colids, dim, option, iters, batch, loss_every, params=(), selftest=False):
    eng = F.Engine(rowptr, colids, dim, selftest=selftest)
    try:
        for k, v in params:
            eng.set_param(k, v)
        eng.set_param("loss_every", loss_every)
        eng.srand(1)
        eng.init_embeddings(0 if option in (5, 8, 11) else 1)
        eng.train(option, iters, batch, 5, 0.02)
        log = eng.train_losses()
        info = {k: eng.get_param(k) for k in ("last_train_form", "last_wide_epochs", "last_loss_us")}
        return eng.get_embeddings(), eng.rand_index(1 << 30), log, info
    finally:
        eng.close()


def _expected_epochs(iters, k):
    return [e for e in range(1, iters + 1) if e % k == 0 or e == iters]


NONINTERFERENCE = [  # name, graph, option, iters, batch, k, params, expected launch form (where the dispatch probe allows chaining)
    ("per_minibatch", "rmat16", 5, 3, 65536, 1, (), 0),
    ("chained", "rmat16", 6, 2, 256, 1, (("chain_wide", 0),), 1),
    ("wide_k1", "cora", 5, 64, 256, 1, (), 2),
    ("wide_k5", "cora", 5, 64, 256, 5, (), 2),
    ("wide_k32", "cora", 6, 64, 256, 32, (), 2),
    ("option7", "cora", 7, 4, 256, 1, (), None),
    ("use_graph", "cora", 5, 5, 256, 2, (("use_graph", 1),), 3),
]


@gpu
@pytest.mark.parametrize("name,graph,option,iters,batch,k,params,form", NONINTERFERENCE, ids=[c[0] for c in NONINTERFERENCE])
def test_loss_log_does_not_change_training(name, graph, option, iters, batch, k, params, form):
    if graph == "rmat16":
        from force2vec_amd.graph import rmat_csr
        rowptr, colids = rmat_csr(16, 16, seed=4)
    else:
        rowptr, colids = load_graph(graph)
    X0, r0, log0, info0 = _run(rowptr, colids, 128, option, iters, batch, 0, params)
    X1, r1, (ep, vals), info1 = _run(rowptr, colids, 128, option, iters, batch, k, params)
    assert np.array_equal(X0, X1) and r0 == r1
    assert len(log0[0]) == 0 and info0["last_loss_us"] == 0
    assert list(ep) == _expected_epochs(iters, k)
    assert vals.shape == (len(ep), 3) and np.all(np.isfinite(vals)) and info1["last_loss_us"] > 0
    assert np.array_equal(vals[:, 0], vals[:, 1] + vals[:, 2])
    assert info0["last_train_form"] == info1["last_train_form"]
    assert info0["last_wide_epochs"] == info1["last_wide_epochs"]
    if form is not None and _round_robin():
        assert info1["last_train_form"] == form
        if form == 2:
            assert info1["last_wide_epochs"] > 1


@gpu
def test_loss_log_where_the_ring_is_refused(monkeypatch):
    """The one-epoch-per-launch fallback of the wide form (self-test build: F2V_TEST_RING_REFUSE) logs the same values, bit for
    bit, as the multi-epoch launches, and trains the same."""
    rowptr, colids = load_graph("cora")
    res = []
    for refuse in (True, False):
        if refuse:
            monkeypatch.setenv("F2V_TEST_RING_REFUSE", "1")
        else:
            monkeypatch.delenv("F2V_TEST_RING_REFUSE", raising=False)
        for k in (0, 3):
            res.append(_run(rowptr, colids, 64, 5, 10, 256, k, selftest=True))
    for X, r, _, _ in res[1:]:
        assert np.array_equal(X, res[0][0]) and r == res[0][1]
    assert list(res[1][2][0]) == [3, 6, 9, 10]
    assert np.array_equal(res[1][2][1], res[3][2][1])
    if _round_robin():
        assert res[1][3]["last_wide_epochs"] == 1 and res[3][3]["last_wide_epochs"] > 1


@gpu
@pytest.mark.parametrize("graph,option,batch", [("cora", 5, 256), ("rmat16", 6, 65536), ("cora", 7, 256)])
def test_log_entry_equals_objective_after_separate_calls(graph, option, batch):
    if graph == "rmat16":
        from force2vec_amd.graph import rmat_csr
        rowptr, colids = rmat_csr(16, 16, seed=4)
    else:
        rowptr, colids = load_graph(graph)
    init = 0 if option == 5 else 1
    a = F.Engine(rowptr, colids, 128)
    b = F.Engine(rowptr, colids, 128)
    try:
        for e in (a, b):
            e.srand(1)
            e.init_embeddings(init)
        a.set_param("loss_every", 5)
        a.train(option, 10, batch, 5, 0.02)
        ep, vals = a.train_losses()
        assert list(ep) == [5, 10]
        b.train(option, 5, batch, 5, 0.02)
        o1 = b.objective(option, 5)
        b.train(option, 5, batch, 5, 0.02)
        o2 = b.objective(option, 5)
        assert np.array_equal(a.get_embeddings(), b.get_embeddings())
        for m, o in enumerate((o1, o2)):
            assert vals[m].tobytes() == np.array([o.loss, o.attraction, o.repulsion]).tobytes()
        # the log belongs to the last call: a call without it leaves none
        a.set_param("loss_every", 0)
        a.train(option, 1, batch, 5, 0.02)
        assert len(a.train_losses()[0]) == 0
    finally:
        a.close()
        b.close()


@gpu
@pytest.mark.parametrize("option", [5, 6])
def test_loss_goes_down_on_cora(option):
    rowptr, colids = load_graph("cora")
    eng = F.Engine(rowptr, colids, 128)
    try:
        eng.srand(1)
        eng.init_embeddings(0 if option == 5 else 1)
        eng.set_param("loss_every", 299)
        eng.train(option, 300, 384, 5, 0.02)
        ep, vals = eng.train_losses()
        assert list(ep) == [299, 300]
        eng.srand(1)
        eng.init_embeddings(0 if option == 5 else 1)
        eng.set_param("loss_every", 1)
        eng.train(option, 1, 384, 5, 0.02)
        ep1, first = eng.train_losses()
        assert list(ep1) == [1]
        assert vals[-1, 0] < first[0, 0]
    finally:
        eng.close()


@gpu
def test_cli_prints_the_log(tmp_path):
    mtx = golden_graph_path("karate.mtx")
    outs = {}
    for loss in (0, 10):
        d = tmp_path / ("loss%d" % loss)
        d.mkdir()
        r = subprocess.run([CLI, "-input", mtx, "-iter", "25", "-dim", "32", "-output", str(d) + "/", "-loss", str(loss)],
                           capture_output=True, text=True, cwd=d, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        embd = [p for p in os.listdir(d) if p.endswith(".embd")]
        assert len(embd) == 1
        outs[loss] = (r.stdout, open(d / embd[0], "rb").read())
    assert outs[0][1] == outs[10][1]
    assert "LOGLIKELIHOOD" not in outs[0][0]
    lines = [l for l in outs[10][0].splitlines() if ":LOGLIKELIHOOD:" in l]
    rowptr, colids = F.read_mtx(mtx)
    eng = F.Engine(rowptr, colids, 32)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        eng.set_param("loss_every", 10)
        eng.train(5, 25, 384, 5, 0.02)
        ep, vals = eng.train_losses()
    finally:
        eng.close()
    assert lines == ["Iteration:%d :LOGLIKELIHOOD: %s" % (e, "%g" % v) for e, v in zip(ep, vals[:, 0])]
    assert [int(l.split(":")[1].split()[0]) for l in lines] == [10, 20, 25]


@gpu
def test_sharded_training_refuses_the_log():
    rowptr, colids = load_graph("karate")
    eng = F.Engine(rowptr, colids, 16)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        eng.set_param("loss_every", 1)
        with pytest.raises(F.F2VError) as e:
            eng.train_sharded(5, 2, 16)
        assert e.value.code == _lib.F2V_EINVAL and "loss_every" in str(e.value)
    finally:
        eng.close()
