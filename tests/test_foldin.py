"""GPU fold-in of new vertices into a trained embedding (include/f2v.h: f2v_fold_in; Engine.fold_in; the CLI's -foldin).

Host tests (no GPU): the numpy restatement of the definition (tests/foldin_ref.py) cut into calls with index_base, the range of the
negative samples and of the random initial vectors, the exported symbol and the CLI's help.  -m gpu: every vector bit for bit against
the restatement (both kernels, every option, all three initial vectors, empty / short / long lists with repeated ids); independence of
calls, chunks, handles and tunables; agreement with f2v_minibatch_step itself; non-interference with training; every refusal; the
held-out experiment of DESIGN.md section 15 on cora; the CLI's file."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib
import foldin_ref as R

CLI = os.path.join(ROOT, "bin", "Force2Vec")
gpu = pytest.mark.gpu
N_KARATE = 34
LR = 0.02


def karate():
    return F.read_mtx(golden_graph_path("karate.mtx"))


def new_lists(n, seed=7):
    """9 new vertices: lists of length 0, 1, 2, 17, 63, 64, 65, 130, and 2 with the same id twice (the long ones repeat ids: n = 34)."""
    rng = np.random.default_rng(seed)
    lists = [rng.integers(0, n, size=k).astype(np.uint32) for k in (0, 1, 2, 17, 63, 64, 65, 130)]
    lists.append(np.array([5, 5], dtype=np.uint32))
    return lists


def some_matrix(n, D, seed, unit):
    rng = np.random.default_rng(seed)
    X = rng.random((n, D), dtype=np.float32)
    return X if unit else (2.0 * X - 1.0).astype(np.float32)


# ---- host ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", [5, 6])
def test_restatement_cut_into_calls_equals_one_call(option):
    X = some_matrix(N_KARATE, 16, 3, option == 6)
    lists = new_lists(N_KARATE)
    for kind in (R.INIT_MEAN, R.INIT_RANDOM):
        whole = R.fold_in(option, X, lists, 3, 5, LR, kind, seed=11, index_base=100)
        a = R.fold_in(option, X, lists[:4], 3, 5, LR, kind, seed=11, index_base=100)
        b = R.fold_in(option, X, lists[4:], 3, 5, LR, kind, seed=11, index_base=104)
        assert np.array_equal(whole.view(np.uint32), np.concatenate([a, b]).view(np.uint32))
        # ... and the index is what tells two vertices with the same list apart
        other = R.fold_in(option, X, lists[4:], 3, 5, LR, kind, seed=11, index_base=105)
        assert not np.array_equal(b, other)


def test_sample_ids_are_vertices():
    for n in (1, 2, 34, 2708, (1 << 32) - 1):
        for Q in (0, 1, 12345, (1 << 40) + 3):
            ids = R.negatives(9, Q, 5, 7, 5, n)
            assert ids.dtype == np.uint32 and len(ids) == 5 and all(int(j) < n for j in ids)
    assert len({tuple(R.negatives(9, Q, e, 7, 5, 2708)) for Q in range(8) for e in range(7)}) == 56  # one draw per (vertex, epoch)
    assert R.mix64(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for seed 0


def test_random_vectors_ranges():
    for Q in (0, 3, 1 << 33):
        u = R.random_vector(6, 1, Q, 100)
        t = R.random_vector(5, 1, Q, 100)
        assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all() and ((t >= -1) & (t < 1)).all()
        assert (np.mod(u.astype(np.float64) * 2.0 ** 24, 1.0) == 0).all()  # multiples of 2^-24
        assert (np.mod(t.astype(np.float64) * 2.0 ** 23, 1.0) == 0).all()  # ... of 2^-23
        assert np.array_equal(t, (2.0 * u.astype(np.float64) - 1.0).astype(np.float32))
        assert len(set(u.tolist())) > 90
    assert np.array_equal(R.random_vector(9, 1, 4, 16), R.random_vector(6, 1, 4, 16))
    assert not np.array_equal(R.random_vector(6, 1, 4, 16), R.random_vector(6, 2, 4, 16))


def test_fold_in_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "f2v_fold_in" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "f2v_fold_in" in _lib.SIGNATURES and C.sizeof(_lib.FoldInfo) == 24
    assert (_lib.FOLD_INIT_MEAN, _lib.FOLD_INIT_RANDOM, _lib.FOLD_INIT_GIVEN) == (0, 1, 2)


def test_cli_help_lists_foldin():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    for flag in ("-foldin ", "-foldin-iters ", "-foldin-init "):
        assert "\n" + flag in r.stdout, flag


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trained(math, D):
    """karate after 3 epochs of option 5 or 6 -> (rowptr, colids, X); shared, never modified"""
    rowptr, colids = karate()
    eng = F.Engine(rowptr, colids, D)
    eng.srand(1)
    eng.init_embeddings(F._lib.INIT_SYMMETRIC if math == 5 else F._lib.INIT_UNIT)
    eng.train(math, 3, 16, 5, LR)
    X = eng.get_embeddings()
    eng.close()
    X.setflags(write=False)
    return rowptr, colids, X


def engine_with(math, D):
    rowptr, colids, X = trained(math, D)
    eng = F.Engine(rowptr, colids, D)
    eng.set_embeddings(X)
    return eng, X


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


KINDS = {"mean": R.INIT_MEAN, "random": R.INIT_RANDOM}


@gpu
@pytest.mark.parametrize("D", [16, 50, 100, 128, 256])  # (50: the generic kernel; 100: the quarter-wave kernel short of its width)
@pytest.mark.parametrize("math", [5, 6])
def test_bit_exact_against_restatement(math, D):
    eng, X = engine_with(math, D)
    lists = new_lists(N_KARATE)
    given = some_matrix(len(lists), D, 21, math == 6)
    for option in (R.T_OPTIONS if math == 5 else R.SIGMOID_OPTIONS):
        for iters in (1, 7):
            for ns in (0, 5):
                for init in ("mean", "random", given):
                    kind = R.INIT_GIVEN if not isinstance(init, str) else KINDS[init]
                    seed, base = 3 + option, 1000 * iters + ns
                    got, info = eng.fold_in(lists, None, option, iters, ns, LR, init, seed, base, details=True)
                    want = R.fold_in(option, X, lists, iters, ns, LR, kind, seed, base, given)
                    assert np.array_equal(bits(got), bits(want)), (option, iters, ns, kind, np.argwhere(bits(got) != bits(want))[:4])
                    assert info.pairs == sum(len(l) + ns for l in lists) * iters and info.seconds > 0
    # iters = 0 returns the initial vectors
    for init, kind in (("mean", R.INIT_MEAN), ("random", R.INIT_RANDOM)):
        got = eng.fold_in(lists, None, math, 0, 5, LR, init, 5, 77)
        want = np.stack([R.initial_vector(math, X, l, kind, 5, 77 + q) for q, l in enumerate(lists)])
        assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(eng.fold_in(lists, None, math, 0, 5, LR, given)), bits(given))
    eng.close()


def resident_is_kept(eng):
    try:
        eng.set_param("fold_resident", 1)
    except _lib.F2VError:
        return False
    eng.set_param("fold_resident", -1)
    return True


@gpu
@pytest.mark.parametrize("math,D", [(5, 128), (6, 128), (5, 16), (6, 256), (5, 100), (6, 50)])
def test_invariance(math, D):
    eng, X = engine_with(math, D)
    lists = new_lists(N_KARATE)
    args = dict(option=math, iters=7, ns=5, lr=LR, init="mean", seed=4)
    base = eng.fold_in(lists, None, index_base=50, **args)
    assert np.array_equal(bits(base), bits(R.fold_in(math, X, lists, 7, 5, LR, R.INIT_MEAN, 4, 50)))
    # two calls with index_base; CSR-like input with a first offset that is not 0
    two = np.concatenate([eng.fold_in(lists[:4], None, index_base=50, **args), eng.fold_in(lists[4:], None, index_base=54, **args)])
    assert np.array_equal(bits(two), bits(base))
    rowptr = np.cumsum([3] + [len(l) for l in lists]).astype(np.uint32)
    colids = np.concatenate([np.zeros(3, dtype=np.uint32)] + lists)
    assert np.array_equal(bits(eng.fold_in(rowptr, colids, index_base=50, **args)), bits(base))
    settings = [("fold_chunk", 4), ("quarter_wave", 0), ("quarter_wave", 1), ("fold_resident", 0), ("waves_per_block", 1), ("waves_per_block", 2)]
    if resident_is_kept(eng):
        settings.append(("fold_resident", 1))
    for name, value in settings:
        before = eng.get_param(name)
        eng.set_param(name, value)
        got, info = eng.fold_in(lists, None, index_base=50, details=True, **args)
        assert np.array_equal(bits(got), bits(base)), (name, value)
        if name == "fold_resident":
            eng.set_param("fold_chunk", 4)  # ... and with chunks of short lists beside chunks of long ones: launches of both forms
            got, info = eng.fold_in(lists, None, index_base=50, details=True, **args)
            assert np.array_equal(bits(got), bits(base)) and info.resident == (value == 1 and D % 4 == 0)
            eng.set_param("fold_chunk", 65536)
        eng.set_param(name, before)
    other, _ = engine_with(math, D)
    assert np.array_equal(bits(other.fold_in(lists, None, index_base=50, **args)), bits(base))
    other.close()
    eng.close()


@gpu
@pytest.mark.parametrize("option", [5, 6])
def test_agrees_with_training_itself(option):
    D, ns = 128, 5
    rowptr, colids, X = trained(option, D)
    deg = np.diff(rowptr.astype(np.int64))
    by_deg = np.argsort(deg, kind="stable")
    twin, _ = engine_with(option, D)
    for i in (int(by_deg[0]), int(by_deg[len(by_deg) // 2]), int(by_deg[-1])):
        row = colids[rowptr[i]:rowptr[i + 1]]
        assert i not in row
        base = 900 + i
        ids = R.negatives(6, base, 0, 1, ns, N_KARATE)
        eng, _ = engine_with(option, D)
        eng.set_param("hub_chunk", 0)
        eng.minibatch_step(option, 0, N_KARATE, ids, ns, LR)
        staged = eng.stage_read(i, i + 1)
        eng.close()
        folded = twin.fold_in([row], None, option, 1, ns, LR, X[i:i + 1], 6, base)
        assert np.array_equal(bits(staged), bits(folded)), i
    twin.close()


@gpu
@pytest.mark.parametrize("option", [5, 6])
def test_purity(option):
    D = 128
    rowptr, colids, X = trained(option, D)
    lists = new_lists(N_KARATE)
    engines = []
    for _ in range(2):
        eng = F.Engine(rowptr, colids, D)
        eng.srand(5)
        eng.set_embeddings(X)
        engines.append(eng)
    a, b = engines
    folded = a.fold_in(lists, None, option, 7, 5, LR)
    assert np.array_equal(bits(a.get_embeddings()), bits(X))
    assert a.rand_index(N_KARATE - 1) == b.rand_index(N_KARATE - 1)
    a.train(option, 5, 16, 5, LR)
    a.fold_in(lists, None, option, 2, 5, LR, "random")
    b.train(option, 5, 16, 5, LR)
    assert np.array_equal(bits(a.get_embeddings()), bits(b.get_embeddings()))
    # a staged minibatch that is not flushed is committed first
    ids = np.array([1, 2, 3, 4, 5], dtype=np.uint32)
    a.minibatch_step(option, 0, 16, ids, 5, LR)
    b.minibatch_step(option, 0, 16, ids, 5, LR)
    b.flush()
    after_a = a.fold_in(lists, None, option, 7, 5, LR)
    after_b = b.fold_in(lists, None, option, 7, 5, LR)
    assert np.array_equal(bits(after_a), bits(after_b)) and not np.array_equal(bits(after_a), bits(folded))
    assert np.array_equal(bits(after_a), bits(R.fold_in(option, b.get_embeddings(), lists, 7, 5, LR)))
    a.close()
    b.close()


def raw_fold(eng, option, rowptr, colids, m, iters, ns, kind, init, seed, base, y):
    ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
    return eng._L.f2v_fold_in(eng._h, option, ptr(rowptr, _lib.u32p), ptr(colids, _lib.u32p), m, iters, ns, LR, kind, ptr(init, _lib.f32p), seed, base,
                              ptr(y, _lib.f32p), None)


@gpu
def test_refusals():
    D = 16
    eng, X = engine_with(5, D)
    rowptr = np.array([0, 2, 3], dtype=np.uint32)
    colids = np.array([1, 2, 3], dtype=np.uint32)
    y = np.full((2, D), 7.0, dtype=np.float32)
    ok = lambda **kw: raw_fold(eng, **{**dict(option=5, rowptr=rowptr, colids=colids, m=2, iters=2, ns=5, kind=0, init=None, seed=1, base=0, y=y), **kw})  # noqa: E731
    assert ok() == _lib.F2V_OK and not (y == 7.0).any()
    for option in (1, 3, 7, 10, 0, 12):
        assert ok(option=option) == _lib.F2V_EINVAL, option
    assert ok(colids=np.array([1, 2, N_KARATE], dtype=np.uint32)) == _lib.F2V_EINVAL
    assert ok(colids=np.array([1, 2, N_KARATE - 1], dtype=np.uint32)) == _lib.F2V_OK
    assert ok(rowptr=np.array([0, 3, 2], dtype=np.uint32)) == _lib.F2V_EINVAL
    assert ok(kind=_lib.FOLD_INIT_GIVEN) == _lib.F2V_EINVAL
    assert ok(kind=_lib.FOLD_INIT_GIVEN, init=np.zeros((2, D), dtype=np.float32)) == _lib.F2V_OK
    assert ok(kind=3) == _lib.F2V_EINVAL and ok(kind=-1) == _lib.F2V_EINVAL
    assert ok(rowptr=None) == _lib.F2V_EINVAL and ok(colids=None) == _lib.F2V_EINVAL and ok(y=None) == _lib.F2V_EINVAL
    # (index_base + m) * iters * ns must stay below 2^62
    assert ok(base=(1 << 62) - 2, iters=1, ns=1) == _lib.F2V_EINVAL
    assert ok(base=(1 << 62) - 3, iters=1, ns=1) == _lib.F2V_OK
    assert ok(base=(1 << 60), iters=2, ns=2) == _lib.F2V_EINVAL
    assert ok(base=(1 << 63), iters=1 << 31, ns=1 << 31) == _lib.F2V_EINVAL
    assert ok(base=(1 << 63), iters=2, ns=0) == _lib.F2V_OK
    with pytest.raises(_lib.F2VError) as ex:
        eng.fold_in([[1, 2]], None, option=7)
    assert ex.value.code == _lib.F2V_EINVAL and "option 7" in str(ex.value)
    with pytest.raises(ValueError):
        eng.fold_in([[1, 2]], None, init="median")
    with pytest.raises(ValueError):
        eng.fold_in([[1, 2]], None, init=np.zeros((2, D), dtype=np.float32))
    # m = 0: F2V_OK, nothing touched -- not even a pending minibatch
    eng.minibatch_step(5, 0, 16, np.array([1, 2, 3, 4, 5], dtype=np.uint32), 5, LR)
    assert raw_fold(eng, 5, None, None, 0, 2, 5, 0, None, 1, 0, None) == _lib.F2V_OK
    assert eng.fold_in([], None).shape == (0, D)
    assert np.array_equal(bits(eng.stage_read(0, 16)), bits(eng.stage_read(0, 16))) and not np.array_equal(bits(eng.stage_read(0, 16)), bits(X[:16]))
    eng.close()
    # before embeddings exist
    fresh = F.Engine(*karate(), D)
    assert raw_fold(fresh, 5, rowptr, colids, 2, 2, 5, 0, None, 1, 0, y) == _lib.F2V_ESTATE
    assert raw_fold(fresh, 5, None, None, 0, 2, 5, 0, None, 1, 0, None) == _lib.F2V_ESTATE
    fresh.close()


# ---- it does what it is for: the held-out experiment of DESIGN.md section 15 -------------------------------------------------------
def cora_labels(n):
    lab = np.full(n, -1, dtype=np.int64)
    for line in open(os.path.join(GOLD, "cora.nodes.labels")):
        t = line.split()
        if len(t) >= 2 and lab[int(t[0]) - 1] < 0:
            lab[int(t[0]) - 1] = int(t[1])
    return lab


def train_cora(rowptr, colids, option):
    eng = F.Engine(rowptr, colids, 128)
    eng.srand(1)
    eng.init_embeddings(F._lib.INIT_SYMMETRIC if option == 5 else F._lib.INIT_UNIT)
    eng.train(option, 1200, 256, 5, LR)
    return eng


def held_out_split(rowptr, colids):
    """-> held, kept, rowptr and colids of the graph without the held-out vertices, the held-out vertices' lists in that graph's ids"""
    n = len(rowptr) - 1
    held = np.random.RandomState(0).permutation(n)[:n // 10]
    is_held = np.zeros(n, dtype=bool)
    is_held[held] = True
    kept = np.flatnonzero(~is_held)
    new_id = np.full(n, -1, dtype=np.int64)
    new_id[kept] = np.arange(len(kept))
    rows = [new_id[colids[rowptr[v]:rowptr[v + 1]]] for v in range(n)]
    rows = [r[r >= 0].astype(np.uint32) for r in rows]
    sub_rowptr = np.concatenate([[0], np.cumsum([len(rows[v]) for v in kept])]).astype(np.uint32)
    sub_colids = np.concatenate([rows[v] for v in kept]).astype(np.uint32)
    return held, kept, sub_rowptr, sub_colids, [rows[v] for v in held]


@gpu
@pytest.mark.parametrize("option", [5, 6])
def test_held_out_vertices_are_classified(option):
    """acc(folded in, mean start) > (acc(random initial vectors) + acc(jointly trained)) / 2 on cora's held-out tenth.
    Measured on an MI355X: option 5: folded 0.826, random initial vectors 0.189, jointly trained 0.867 (0.826 > 0.528); option 6: folded
    0.593, random initial vectors 0.133, jointly trained 0.663 (0.593 > 0.398); folded from a random start (reported, not asserted):
    0.756 and 0.252."""
    from sklearn.linear_model import LogisticRegression
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    lab = cora_labels(len(rowptr) - 1)
    held, kept, sub_rowptr, sub_colids, lists = held_out_split(rowptr, colids)
    joint = train_cora(rowptr, colids, option)
    XJ = joint.get_embeddings()
    joint.close()
    eng = train_cora(sub_rowptr, sub_colids, option)
    XK = eng.get_embeddings()
    folded = eng.fold_in(lists, None, option, 600, 5, LR, "mean", 1)
    initial = eng.fold_in(lists, None, option, 0, 5, LR, "random", 1)
    from_random = eng.fold_in(lists, None, option, 600, 5, LR, "random", 1)
    eng.close()
    model = LogisticRegression(max_iter=1000).fit(XK.astype(np.float64), lab[kept])
    acc = {name: float(model.score(Y.astype(np.float64), lab[held])) for name, Y in (("folded", folded), ("initial", initial), ("from_random", from_random))}
    acc["joint"] = float(LogisticRegression(max_iter=1000).fit(XJ[kept].astype(np.float64), lab[kept]).score(XJ[held].astype(np.float64), lab[held]))
    print("fold-in cora option %d: folded %.3f, initial random vectors %.3f, jointly trained %.3f, folded from a random start %.3f"
          % (option, acc["folded"], acc["initial"], acc["joint"], acc["from_random"]))
    assert acc["folded"] > (acc["initial"] + acc["joint"]) / 2, acc


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_cli_foldin(tmp_path):
    lines = [("alice", [1, 2, 3]), ("bob", []), ("v35", [34, 34, 7, 9, 12])]
    with open(tmp_path / "new.txt", "w") as f:
        for name, ids in lines:
            f.write(" ".join([name] + [str(i) for i in ids]) + "\n")
    r = subprocess.run([CLI, "-input", golden_graph_path("karate.mtx"), "-output", str(tmp_path) + "/", "-iter", "3", "-batch", "16", "-dim", "16", "-option", "6",
                        "-binout", "1", "-seed", "3", "-foldin", str(tmp_path / "new.txt"), "-foldin-iters", "5"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    embd = [ln.split(":", 1)[1].strip() for ln in r.stdout.splitlines() if ln.startswith("Creating output file in following directory:")][0]
    assert "Fold-in: 3 vertices, 5 iterations" in r.stdout
    rows = [ln.split() for ln in open(embd + ".fold")]
    assert rows[0] == ["3", "16"] and len(rows) == 4 and [row[0] for row in rows[1:]] == [name for name, _ in lines]
    assert all(len(row) == 17 for row in rows[1:])
    rowptr, colids = karate()
    eng = F.Engine(rowptr, colids, 16)
    eng.set_embeddings(F.read_embd_bin(embd + ".bin", N_KARATE, 16))
    want = eng.fold_in([[i - 1 for i in ids] for _, ids in lines], None, 6, 5, 5, LR, "mean", 3)
    eng.close()
    for row, w in zip(rows[1:], want):
        assert [float(t) for t in row[1:]] == [float("%g" % v) for v in w]
    # what does not fold in is refused before the graph is read
    r = subprocess.run([CLI, "-input", "/nonexistent.mtx", "-option", "7", "-foldin", "x"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "-foldin is available with options 5, 6, 8, 9 and 11" in r.stdout
    r = subprocess.run([CLI, "-input", "/nonexistent.mtx", "-foldin", "x", "-foldin-init", "median"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "-foldin-init must be mean or random" in r.stdout
