"""The step, exact, fold-in and objective kernels at the values where fp32 and fp64 arithmetic can differ between two correct-looking
instruction sequences (tests/extreme_values.py: the planted rows, the comparison, the hand-derived rules; DESIGN.md "Special values").

Host tests (no GPU): the oracle's single interaction equals the rules on every special case, in both orders; the numpy restatements
take the planted matrices and obey the rules; the runs the GPU tests compare against say something (most rows finite, a subnormal
coefficient in the first minibatch, ...); the two extended-precision references of the objective's terms agree.
-m gpu: every launch form of the interaction against the oracle / the restatements on those matrices -- one minibatch at a time,
f2v_train's forms, option 1, the fold-in -- and the objective one pair at a time against 50 digits.  Every comparison is
extreme_values.same_values: a NaN where a NaN is expected, identical bits everywhere else."""
import functools
import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLD

import force2vec_amd as F
from oracle import oracle as O
import exact_ref
import extreme_values as E
import foldin_ref
from test_objective import objective_ref, pair_scalars_kernel_order

gpu = pytest.mark.gpu
N, NS, LR, BATCH, CHUNK = 256, 5, 0.02, E.BATCH, E.HUB_CHUNK
F32, F64 = np.float32, np.float64
DIMS = (16, 100, 128, 256)
# The seed of the planted matrix, by D: chosen on the CPU so that the conditions below hold on the oracle's results (an option 6 run in
# which a huge row is drawn as a shared sample early ends with most entries above 1e6 -- a matrix that says nothing any more;
# at D = 16 the two "1e9" rows must also lie far enough apart for their coefficient to be subnormal: a > 1.3e19).
SEEDS = {3: 3, 16: 20, 100: 4}


def seed_of(D):
    return SEEDS.get(D, 5)


@functools.lru_cache(maxsize=None)
def graph(n=N):
    rowptr, colids = E.planted_graph(n)
    rowptr.setflags(write=False)
    colids.setflags(write=False)
    return rowptr, colids


def start(D, nonfinite, n=N):
    X, classes = E.planted(n, D, seed_of(D), nonfinite)
    X.setflags(write=False)
    return X, classes


def ok(got, want, classes=None, rows=None, what=""):
    assert E.same_values(got, want), what + ": " + E.difference(got, want, classes, rows)


# ---- what the expected results must show, so that a test does not pass on a matrix that says nothing ---------------------------------
def readers_of(rows, n=N):
    rowptr, colids = graph(n)
    hit = np.isin(colids, rows)
    return np.unique(np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))[hit])


def conditions(want, classes, option, nonfinite, small=False):
    """On an expected matrix: at least half the rows are entirely finite; where non-finite values were planted, a reader of such a row
    has stayed finite and -- sigmoid options -- an ordinary row has become non-finite (the t-distribution options cannot: the clamp
    turns every NaN force into -5, so there NO ordinary row may); small: at least half the entries stay below 1e6 in magnitude."""
    finite = np.isfinite(want).all(axis=1)
    assert finite.mean() >= 0.5, finite.mean()
    if nonfinite:
        planted = sorted(r for rows in classes.values() for r in rows)
        ordinary = np.ones(len(want), dtype=bool)
        ordinary[planted] = False
        bad = [r for name, _ in E.NONFINITE_CLASSES for r in classes[name]]
        readers = [r for r in readers_of(bad, len(want)) if r not in bad]
        assert len(readers) and finite[readers].any()
        if option in (1, 5):
            assert finite[ordinary].all()
        else:
            assert not finite[ordinary].all()
    if small:
        with np.errstate(invalid="ignore"):
            assert (np.abs(want) < 1e6).mean() >= 0.5, (np.abs(want) < 1e6).mean()


# ---- (a) one minibatch at a time: the oracle's side, computed once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_steps(option, D, bs, nonfinite, epochs):
    """-> dict: X0, classes, plan [(lo, hi, ids)], states [the matrix after every minibatch], walks [per epoch], checks [(step, row,
    the row by expected_row)] for the planted rows whose every interaction in that minibatch is a special case."""
    rowptr, colids = graph()
    X0, classes = start(D, nonfinite)
    plan = E.minibatch_plan(N, option, bs, epochs, classes, nonfinite)
    per_epoch = len(plan) // epochs
    planted = sorted(r for rows in classes.values() for r in rows)
    X, orng, states, walks, checks = X0.copy(), O.Rng(3), [], [], []
    for k, (lo, hi, ids) in enumerate(plan):
        if option == 7 and k % per_epoch == 0:
            walks.append(O.generate_walks(orng, rowptr, colids))
        w = walks[-1] if option == 7 else None
        before = X.copy()
        O.minibatch(option, rowptr, colids, X, lo, hi, ids, NS, LR, bs_mode=bs, walks=w, order=O.ORDER_TREE, chunk=CHUNK)
        states.append(X.copy())
        for p in planted:
            deg = int(rowptr[p + 1] - rowptr[p])
            if not lo <= p < hi or deg > CHUNK:
                continue
            nbrs = w[5 * p:5 * p + 5] if option == 7 else colids[rowptr[p]:rowptr[p + 1]]
            try:
                checks.append((k, p, E.expected_row(option, before, p, nbrs, ids[p - lo:p - lo + NS] if bs else ids[:NS], LR, degree=deg)))
            except E.NotSpecial:
                pass
    return dict(X0=X0, classes=classes, plan=plan, states=states, walks=walks, checks=checks, per_epoch=per_epoch)


def passes_of(option):
    """(nonfinite, epochs): option 5 keeps most rows finite whatever it reads (NaN -> -5) and runs the non-finite rows for two epochs;
    a sigmoid option turns every reader of a NaN to NaN, so it takes them for one pass and the finite classes for two epochs."""
    return ((True, 2),) if option == 5 else ((True, 1), (False, 2))


# (option 7 has no -bs 1 form: the library and the oracle refuse it, oracle/f2v_oracle.c orc_train)
STEP_KEYS = [(option, D, bs) for option in (5, 6, 7) for D in DIMS + (3, 101) for bs in (0, 1) if not (option == 7 and bs)]


# ---- host --------------------------------------------------------------------------------------------------------------------------
def test_sigmoid_table_restatement():
    """extreme_values' own table (float x, expf, 1.0 / (float) in double, narrowed) is the oracle's, and the cell values sit where
    fast_SM's index changes: the oracle returns table[c - 1] below and table[c] above each boundary."""
    table = O.sm_table()
    assert E.same_values(E.sm_table(), table)
    vals = E.cell_values()
    for c, lo, hi in zip(E.CELLS, vals[0::2], vals[1::2]):
        assert hi == np.nextafter(lo, F32(np.inf))
        assert O.lib().orc_fast_sm(O._f32(table), float(lo)) == table[c - 1] != table[c] == O.lib().orc_fast_sm(O._f32(table), float(hi))
    fast = lambda v: O.lib().orc_fast_sm(O._f32(table), float(F32(v)))  # noqa: E731
    six = F32(6.0)
    assert fast(six) == table[2047] and fast(np.nextafter(six, F32(7))) == 1.0
    assert fast(-six) == table[0] and fast(np.nextafter(-six, F32(-7))) == 0.0 and fast(np.nan) == table[0]


def special_cases(D, rng):
    """(name, option, xi, xj, negative sample?) -- every one a case expected_pair must decide"""
    k, last = min(1, D - 1), D - 1
    u = rng.uniform(-1, 1, D).astype(F32)
    v = rng.uniform(-1, 1, D).astype(F32)
    u[k] = abs(u[k]) + F32(0.25)

    def with_(x, d, val):
        y = x.copy()
        y[d] = val
        return y

    def hot(val):
        y = np.zeros(D, dtype=F32)
        y[0] = val
        return y

    with np.errstate(all="ignore"):
        tiny = (u * F32(1e-20)).astype(F32)
        huge = (F32(3e19) * np.sign(u)).astype(F32)
        sub, sub2 = (u * F32(1e-40)).astype(F32), (v * F32(1e-40)).astype(F32)
    three = F32(3.0)
    cases = []
    for neg in (True, False):
        cases += [("a = 0", 5, u, u.copy(), neg), ("rows of -0.0", 5, np.full(D, -0.0, dtype=F32), np.full(D, -0.0, dtype=F32), neg),
                  ("a = inf from finite rows", 5, u, huge, neg), ("a = inf from finite rows, the row itself huge", 5, huge, v, neg),
                  ("+inf in the other row", 5, u, with_(v, k, np.inf), neg), ("-inf in the last dimension", 5, u, with_(v, last, -np.inf), neg),
                  ("inf in the row itself", 5, with_(u, k, np.inf), v, neg), ("inf in both, different signs", 5, with_(u, k, np.inf), with_(v, k, -np.inf), neg),
                  ("inf in both, the same: inf - inf", 5, with_(u, k, np.inf), with_(v, k, np.inf), neg),
                  ("a NaN row", 5, u, np.full(D, np.nan, dtype=F32), neg), ("one NaN", 5, u, with_(v, k, np.nan), neg),
                  ("one NaN in the row itself", 5, with_(u, k, np.nan), v, neg)]
    cases += [("one ulp apart, the square underflows (+)", 5, with_(tiny, k, np.nextafter(tiny[k], F32(1))), tiny, True),
              ("one ulp apart, the square underflows (-)", 5, tiny, with_(tiny, k, np.nextafter(tiny[k], F32(1))), True),
              ("one ulp apart, a normal square (+)", 5, with_(u, k, np.nextafter(u[k], F32(2))), u, True),
              ("one ulp apart, a normal square (-)", 5, u, with_(u, k, np.nextafter(u[k], F32(2))), True),
              ("subnormal rows", 5, sub, sub2, True), ("equal subnormal rows", 5, sub, sub.copy(), False)]
    big = (u * F32(1e9)).astype(F32)
    for neg in (True, False):
        cases += [("dot just above 6", 6, hot(2), hot(np.nextafter(three, F32(4))), neg), ("dot = 6.0f", 6, hot(2), hot(3), neg),
                  ("dot just below 6", 6, hot(2), hot(np.nextafter(three, F32(2))), neg), ("dot = -6.0f", 6, hot(2), hot(-3), neg),
                  ("dot just below -6", 6, hot(2), hot(-np.nextafter(three, F32(4))), neg), ("dot = 0", 6, hot(2), with_(np.zeros(D, dtype=F32), last, 0.0), neg),
                  ("dot far above 6", 6, big, big.copy(), neg), ("dot far below -6", 6, big, -big, neg),
                  ("a NaN dot", 6, u, with_(v, k, np.nan), neg), ("a NaN row", 6, u, np.full(D, np.nan, dtype=F32), neg),
                  ("dot = +inf: sm = 1 and the other row's inf x 0", 6, u, with_(np.abs(v), k, np.inf), neg),
                  ("dot = -inf", 6, u, with_(-np.abs(v), k, -np.inf) if D > 1 else hot(-np.inf), neg)]
        cases += [("cell boundary %d" % i, 6, hot(1), hot(val), neg) for i, val in enumerate(E.cell_values())]
    return cases


def two_vertices(neighbour):
    rowptr = np.array([0, 1, 1] if neighbour else [0, 0, 0], dtype=np.uint32)
    return rowptr, np.array([1], dtype=np.uint32)


@pytest.mark.parametrize("D", [1, 4, 100, 128])
@pytest.mark.parametrize("order", [O.ORDER_TREE, O.ORDER_REF])
def test_oracle_single_interaction_equals_the_rules(D, order):
    """oracle.row / oracle.minibatch on two- and three-vertex graphs against expected_pair / expected_row, both orders of summation."""
    rng = np.random.default_rng(D)
    seen = 0
    for name, option, xi, xj, neg in special_cases(D, rng):
        X = np.ascontiguousarray(np.stack([xi, xj]), dtype=F32)
        rowptr, colids = two_vertices(not neg)
        samples = np.array([1], dtype=np.uint32) if neg else np.zeros(0, dtype=np.uint32)
        want = E.expected_pair(option, neg, xi, xj, LR, E.c0_of(LR, 1))
        got = O.row(option, rowptr, colids, X, 0, samples, LR, order=order)
        ok(got, want, what="%s (option %d, %s)" % (name, option, "repulsion" if neg else "attraction"))
        Xm = X.copy()
        O.minibatch(option, rowptr, colids, Xm, 0, 1, np.array([1], dtype=np.uint32), 1 if neg else 0, LR, order=order)
        ok(Xm[0], want, what=name + " through oracle.minibatch")
        ok(Xm[1], xj, what=name + ": the other row")
        seen += 1
    assert seen == 66
    # three vertices: a neighbour, then a sample, chained by expected_row; and the self-sample (a = 0 from the row itself)
    u = rng.uniform(-1, 1, D).astype(F32)
    nan_row = np.full(D, np.nan, dtype=F32)
    inf_row = u.copy()
    inf_row[D - 1] = np.inf
    rowptr, colids = np.array([0, 1, 1, 1], dtype=np.uint32), np.array([1], dtype=np.uint32)
    for a, b in ((u.copy(), nan_row), (nan_row, inf_row), (inf_row, u.copy()), (u.copy(), u.copy())):
        X = np.ascontiguousarray(np.stack([u, a, b]), dtype=F32)
        for samples in ([2], [0], [2, 0, 1]):
            got = O.row(5, rowptr, colids, X, 0, np.array(samples, dtype=np.uint32), LR, order=order)
            ok(got, E.expected_row(5, X, 0, [1], samples, LR), what="three vertices, samples %s" % samples)
    hot = np.zeros((3, D), dtype=F32)
    hot[:, 0] = (2, 3, -3)
    got = O.row(6, rowptr, colids, hot, 0, np.array([2, 1], dtype=np.uint32), LR, order=order)
    ok(got, E.expected_row(6, hot, 0, [1], [2, 1], LR), what="three one-hot vertices")


def test_expected_pair_refuses_ordinary_pairs():
    rng = np.random.default_rng(0)
    u, v = rng.uniform(-1, 1, 16).astype(F32), rng.uniform(-1, 1, 16).astype(F32)
    for option, neg in ((5, True), (5, False), (6, True), (6, False)):
        with pytest.raises(E.NotSpecial):
            E.expected_pair(option, neg, u, v, LR, E.c0_of(LR, 3))


def test_same_values_and_its_message():
    a = np.array([[0.0, np.nan, np.inf], [1.0, -0.0, 2.0]], dtype=F32)
    b = a.copy()
    b[0, 1] = -np.nan  # another NaN: the same value
    assert E.same_values(a, b) and E.difference(a, b) == "same values"
    for (r, d), val in (((1, 1), 0.0), ((0, 2), -np.inf), ((0, 1), 1.0), ((1, 0), np.nan), ((1, 2), np.nextafter(F32(2), F32(3)))):
        c = a.copy()
        c[r, d] = val
        assert not E.same_values(c, a) and not E.same_values(a, c)
        msg = E.difference(c, a, {"equal": [r + 10]}, rows=[10, 11])
        assert "(row %d, dim %d)" % (r + 10, d) in msg and "class 'equal'" in msg and "0x%08x" % int(c.view(np.uint32)[r, d]) in msg


def test_planted_rows_and_graph():
    """Every class is where the dict says, the graph reads every planted row in all three roles' lists, ascending inside a row."""
    for n in (N, 1100):
        rowptr, colids = graph(n)
        X, classes = E.planted(n, 16, 1, True)
        assert int(rowptr[-1]) == len(colids) and colids.max() < n
        assert all(np.all(np.diff(colids[rowptr[i]:rowptr[i + 1]].astype(np.int64)) >= 0) for i in range(n))
        rows = sorted(r for rs in classes.values() for r in rs)
        assert len(rows) == len(set(rows)) == 32 and 5 not in rows and n - 3 not in rows
        deg = np.diff(rowptr.astype(np.int64))
        assert deg[5] > 4 * CHUNK and deg[n - 3] > 4 * CHUNK and deg[n - 2] >= 32  # split into pieces
        for p in rows:
            assert 1 <= deg[p] <= CHUNK                                           # a batch row of one piece
            readers = readers_of([p], n)
            assert p + 3 in readers and n - 2 in readers                          # an ordinary row and a split row read it
        a, b = classes["equal"]
        assert X[a].tobytes() == X[b].tobytes()
        base, moved = classes["ulp"]
        assert (X[base] != X[moved]).sum() == 1
        assert np.isnan(X[classes["nan_row"][0]]).all() and np.isnan(X[classes["nan_one"][0]]).sum() == 1
        assert X[classes["ninf_last"][0], -1] == -np.inf and np.isposinf(X[classes["inf_one"][0]]).sum() == 1
        assert np.signbit(X[classes["negzero"][0]]).all() and not X[classes["negzero"][0]].any()
        assert 0 < np.abs(X[classes["1e-40"][0]]).max() < E.FLT_MIN
        hot = X[classes["onehot"], 0]
        assert hot[0] * hot[1] == 6 and hot[0] * hot[2] > 6 and hot[0] * hot[3] < 6 and hot[0] * hot[4] == -6
        assert np.isfinite(E.planted(n, 16, 1, False)[0]).all()
    assert max(E.class_rows(1100)["1e19"]) >= 1024  # beyond the first span of option 1's columns


@pytest.mark.parametrize("option,D,bs", STEP_KEYS)
def test_minibatch_runs_say_something(option, D, bs):
    """The conditions on the oracle's results of (a), and the oracle itself against the rules on the rows the rules decide."""
    total = 0
    for nonfinite, epochs in passes_of(option):
        ref = oracle_steps(option, D, bs, nonfinite, epochs)
        conditions(ref["states"][-1], ref["classes"], option, nonfinite)
        for k, p, want in ref["checks"]:
            ok(ref["states"][k][p], want, ref["classes"], rows=[p], what="minibatch %d, row %d by the rules" % (k, p))
        total += len(ref["checks"])
        if option == 5 and D >= 16:
            # the first "1e9" row meets the second one as a sample in the very first minibatch: a subnormal coefficient
            a, b = ref["classes"]["1e9"]
            lo, hi, ids = ref["plan"][0]
            assert lo <= a < hi and b in (ids[a - lo:a - lo + NS] if bs else ids[:NS])
            assert E.is_subnormal(E.rep_coef(ref["X0"][a], ref["X0"][b]))
    assert total >= 8


# D = 3 and 101: the generic kernel, which f2v_train launches one minibatch at a time only (the chained forms are the sub-wave layout's)
TRAIN_KEYS = [(option, D, fanin) for option in (5, 6, 7) for D in DIMS + (3, 101) for fanin in (2, 32)]


@functools.lru_cache(maxsize=None)
def oracle_train(option, D, fanin):
    rowptr, colids = graph()
    nonfinite, epochs = (True, 3) if option == 5 else (False, 2)
    X0, classes = start(D, nonfinite)
    O.set_fanin(fanin)
    try:
        want = O.train(option, rowptr, colids, D, epochs, BATCH, X0=X0, order=O.ORDER_TREE, chunk=CHUNK)
    finally:
        O.set_fanin(32)
    want.setflags(write=False)
    return X0, classes, want, epochs, nonfinite


@pytest.mark.parametrize("option,D,fanin", TRAIN_KEYS)
def test_train_runs_say_something(option, D, fanin):
    X0, classes, want, epochs, nonfinite = oracle_train(option, D, fanin)
    conditions(want, classes, option, nonfinite, small=option != 5)
    assert not E.same_values(want, X0)
    if option == 5 and D >= 100:
        # the first minibatch's shared samples are the first five rand() draws: against any ordinary row the first "1e9" row's a is about
        # D / 3 * 1e18, so from D = 100 on its coefficient is subnormal (D = 16: 7e-38, normal -- there only the minibatch runs, which
        # choose the second "1e9" row as the sample, reach one)
        rng, first = O.Rng(1), classes["1e9"][0]
        ids = [rng.rand_index(N - 1) for _ in range(NS)]
        assert first < BATCH and any(E.is_subnormal(E.rep_coef(X0[first], X0[j])) for j in ids)
    if fanin == 32:  # both orders take such matrices and agree on what is finite
        ref = O.train(option, *graph(), D, epochs, BATCH, X0=X0, order=O.ORDER_REF)
        assert np.array_equal(np.isnan(ref), np.isnan(want))


def exact_small(xi, xj):
    """exact_ref on the two-vertex graph without an edge: row 0 takes the repulsion of column 1 with STEP = 1"""
    X = np.ascontiguousarray(np.stack([xi, xj]), dtype=F32)
    return exact_ref.train(X, np.zeros(3, dtype=np.uint32), np.zeros(0, dtype=np.uint32), 2, 1, order="engine", threads=1, special_values=True)[0]


def test_restatements_take_the_planted_matrices():
    """exact_ref.train, foldin_ref.fold_in and test_objective.objective_ref on planted matrices with warnings turned into errors, and
    the rules where they apply to them."""
    rowptr, colids = graph()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        X0, classes = start(16, True)
        X = exact_ref.train(X0, rowptr, colids, BATCH, 1, order="engine", special_values=True)
        conditions(X, classes, 1, True)
        lists = fold_lists(classes, True)
        for math in (5, 6):
            res, cl = start(16, math == 5)
            Y = foldin_ref.fold_in(math, res, fold_lists(cl, math == 5), 2, NS, LR, foldin_ref.INIT_MEAN)
            assert np.isfinite(Y).all(axis=1).mean() >= 0.5
        for option in (5, 10):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):  # (what such rows do to numpy is part of the definition)
                att, rep, pos, neg = objective_ref(np.array(X0), rowptr, colids, option, NS)
                assert np.isnan(att) and pos == len(colids)
                att, rep, _, _ = objective_ref(np.array(start(16, False)[0]), rowptr, colids, option, NS)
            assert np.isfinite(att) and np.isfinite(rep)
        # the rules: option 1's repulsion is the t-distribution rule with STEP = 1 in the place of lr ...
        rng = np.random.default_rng(2)
        for name, option, xi, xj, neg in special_cases(16, rng):
            if option == 5 and neg:
                ok(exact_small(xi, xj), xi + (np.zeros(16, dtype=F32) + E.contribution5(True, xi, xj, 1.0)), what="exact_ref: " + name)
        # ... the fold-in of a vertex with one neighbour and a given start is one attraction ...
        for name, option, xi, xj, neg in special_cases(16, rng):
            if not neg:
                Xr = np.ascontiguousarray(np.stack([xj, xj]), dtype=F32)
                got = foldin_ref.fold_in(option, Xr, [[1]], 1, 0, LR, foldin_ref.INIT_GIVEN, given=xi[None, :])[0]
                ok(got, E.expected_pair(option, False, xi, xj, LR, E.c0_of(LR, 1)), what="foldin_ref: " + name)
        # ... and equal rows are a pair scalar of exactly zero: log1p(0) = 0
        eq = np.ascontiguousarray(np.stack([X0[7], X0[7]]), dtype=F32)
        with np.errstate(divide="ignore"):
            att, rep, _, _ = objective_ref(eq, *two_vertices(True), 5, 0)
        assert att == 0.0 and rep == 0.0
    assert len(lists) > 20


# ---- (c) option 1 ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_restated(n, D, epochs):
    rowptr, colids = graph(n)
    X0, classes = start(D, True, n)
    want = exact_ref.train(X0, rowptr, colids, BATCH if n == N else 384, epochs, order="engine", special_values=True)
    want.setflags(write=False)
    return X0, classes, want


@pytest.mark.parametrize("D", DIMS + (3, 101))
def test_exact_runs_say_something(D):
    for epochs in (1, 2):
        X0, classes, want = exact_restated(N, D, epochs)
        conditions(want, classes, 1, True)
        assert not E.same_values(want, X0)


# ---- (d) fold-in --------------------------------------------------------------------------------------------------------------------
def fold_lists(classes, nonfinite):
    """New vertices: one whose list is a whole class, for every class; one that names an ordinary row and one planted row, for every
    class; one that names every planted row (a long list); one without neighbours."""
    names = [name for name, _ in E.FINITE_CLASSES + (E.NONFINITE_CLASSES if nonfinite else ())]
    lists = [np.array(classes[name], dtype=np.uint32) for name in names]
    lists += [np.array([3 + 2 * k, classes[name][-1], 250 - k], dtype=np.uint32) for k, name in enumerate(names)]
    lists.append(np.array(sorted(r for name in names for r in classes[name]) * 3, dtype=np.uint32))
    lists.append(np.zeros(0, dtype=np.uint32))
    return lists


def fold_given(resident, m, D):
    """A start of the caller's own: uniform rows, the first one a duplicate of the resident row the first list names (a = 0)."""
    Y0 = np.random.default_rng(m + D).uniform(-1, 1, (m, D)).astype(F32)
    Y0[0] = resident[7]
    return Y0


@functools.lru_cache(maxsize=None)
def fold_restated(math, D, iters, ns, init):
    resident, classes = start(D, math == 5)
    lists = fold_lists(classes, math == 5)
    given = fold_given(resident, len(lists), D) if init == "given" else None
    want = foldin_ref.fold_in(math, resident, lists, iters, ns, LR, foldin_ref.INIT_GIVEN if init == "given" else foldin_ref.INIT_MEAN, given=given)
    return resident, classes, lists, given, want


FOLD_KEYS = [(math, D, iters, ns) for math in (5, 6) for D in (16, 50, 100, 128) for iters in (1, 7) for ns in (0, 5)]


@pytest.mark.parametrize("math,D,iters,ns", FOLD_KEYS)
def test_fold_in_runs_say_something(math, D, iters, ns):
    for init in ("mean", "given"):
        resident, classes, lists, given, want = fold_restated(math, D, iters, ns, init)
        assert np.isfinite(want).all(axis=1).mean() >= 0.5
        if math == 5:  # the mean of a list with a NaN row is NaN and stays NaN; a finite start stays finite whatever it reads: NaN -> -5
            assert np.isfinite(want).all() == (init == "given")


# ---- (e) the objective, one pair at a time -----------------------------------------------------------------------------------------
Z5 = [0.0, 1e-38, 1e-30, 1e-12, 1e-6, 1.0, 1e6, 1e30, np.inf, np.nan]
Z10 = [s * z for z in (0.0, 1e-30, 1.0, 20.0, 40.0, 100.0, 700.0, 745.0, 1e30, np.inf) for s in (1.0, -1.0)] + [np.nan]
OBJ_D = 64
DBL_MIN = float(np.finfo(F64).tiny)


def pair_rows(z, sigmoid):
    """Two rows of 64 dims whose fp32 pair scalar -- the squared distance, or the dot product -- is exactly float32(z) in every order
    of summation: one dim per set bit 2^p of z holds 2^(p/2) (two dims 2^((p-1)/2) where p is odd), so every term is a power of two
    inside z's 24-bit window and every partial sum is exact; inf and NaN take one dim."""
    z = F32(z)
    a, b = np.zeros(OBJ_D, dtype=F32), np.zeros(OBJ_D, dtype=F32)
    if not np.isfinite(z):
        a[0], b[0] = (1.0, z) if sigmoid else (0.0, z)
        return a, b
    if z == 0:
        if sigmoid:  # every product is a zero of z's sign
            b[:] = -1.0 if np.signbit(z) else 1.0
        return a, b
    m, e = np.frexp(F64(abs(z)))
    bits, e, dims = int(m * 2 ** 24), int(e) - 24, []
    for k in range(24):
        if bits >> k & 1:
            p = e + k
            dims += [2.0 ** (p // 2)] if p % 2 == 0 else [2.0 ** ((p - 1) // 2)] * 2
    assert len(dims) <= OBJ_D
    x = np.zeros(OBJ_D, dtype=F32)
    x[:len(dims)] = dims
    assert (x[:len(dims)].astype(F64) == dims).all()
    if sigmoid:
        return x, (-x if z < 0 else x).astype(F32)
    return a, x


def pair_matrix(z, sigmoid):
    X = np.ascontiguousarray(np.stack(pair_rows(z, sigmoid)), dtype=F32)
    got = pair_scalars_kernel_order(X, np.array([0]), np.array([1]), sigmoid)[0]
    assert E.same_values(got, F32(z)), (z, got)
    return X


def ref_terms(z, precise=True):
    """-> (log1p(z), softplus(-z), the repulsion of the pair graph with ns = 1: -(log(1e-6) - log1p(0)) - (log(1e-6 + z) - log1p(z)),
    that repulsion's unit |log(1e-6 + z)| + |log1p(z)|), z the fp32 value; mpmath at 50 digits, or np.longdouble."""
    z = F64(F32(z))
    if precise:
        import mpmath
        with mpmath.workprec(170):
            x, eps = mpmath.mpf(float(z)), mpmath.mpf(1e-6)
            att5 = mpmath.log1p(x) if x >= 0 or mpmath.isnan(x) else mpmath.nan
            att10 = mpmath.log1p(mpmath.exp(-abs(x))) + max(-x, 0) if not mpmath.isnan(x) else mpmath.nan
            if x >= 0:
                rep5 = -(mpmath.log(eps)) - (mpmath.log(eps + x) - mpmath.log1p(x))
                unit = abs(mpmath.log(eps + x)) + abs(mpmath.log1p(x))
            else:
                rep5 = unit = mpmath.nan
            return tuple(v + 0 for v in (att5, att10, rep5, unit))
    L = np.longdouble
    with np.errstate(all="ignore"):
        x, eps = L(z), L(1e-6)
        att5 = np.log1p(x)
        att10 = np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, L(0))
        rep5 = -np.log(eps) - (np.log(eps + x) - np.log1p(x))
        unit = np.abs(np.log(eps + x)) + np.abs(np.log1p(x))
    return att5, att10, rep5, unit


def have_mpmath():
    try:
        import mpmath  # noqa: F401
        return True
    except ImportError:
        return False


def error_of(got, ref, unit=None):
    """A finite value against the reference: relative (attraction; a reference below the smallest normal double is measured against
    that number -- fp64 holds nothing finer there, exp(-745) is a subnormal of one bit), or in the given unit (repulsion)."""
    if have_mpmath():
        import mpmath
        with mpmath.workprec(170):
            d = abs(mpmath.mpf(float(got)) - ref)
            return float(d / (unit if unit is not None else max(abs(ref), mpmath.mpf(DBL_MIN))))
    d = abs(np.longdouble(got) - ref)
    return float(d / (unit if unit is not None else max(abs(ref), np.longdouble(DBL_MIN))))


def kind(v):
    v = float(v)
    return "nan" if v != v else ("+inf" if v == np.inf else "-inf" if v == -np.inf else "finite")


def test_the_two_objective_references_agree():
    """mpmath at 50 digits and np.longdouble on every z of the lists: the same kind, and 1e-17 apart at the most in the measure the
    GPU test uses (only where both exist)."""
    pytest.importorskip("mpmath")
    import mpmath
    for z in sorted(set(Z5 + Z10), key=lambda v: (v != v, v)):
        hi, lo = ref_terms(z), ref_terms(z, precise=False)
        for k in range(3):
            if k != 1 and z < 0:  # (a squared distance is never negative)
                continue
            assert kind(hi[k]) == kind(lo[k]), (z, k)
            if kind(hi[k]) == "finite":
                with mpmath.workprec(170):
                    m, e = np.frexp(np.longdouble(lo[k]))  # (the long double, exactly: its 64-bit significand as an integer)
                    d = abs(mpmath.ldexp(mpmath.mpf(int(m * np.longdouble(2.0) ** 64)), int(e) - 64) - hi[k])
                    unit = hi[3] if k == 2 else max(abs(hi[k]), mpmath.mpf(DBL_MIN))
                    assert d / unit < 1e-17, (z, k, float(d / unit))


def test_pair_rows_give_the_scalar_exactly():
    for z in Z5:
        pair_matrix(z, False)
    for z in Z10:
        pair_matrix(z, True)
    assert np.signbit(pair_scalars_kernel_order(pair_matrix(-0.0, True), np.array([0]), np.array([1]), True)[0])


def golden_errors():
    with open(os.path.join(GOLD, "extreme_values.json")) as f:
        return json.load(f)


def test_recorded_objective_errors_are_within_the_condition():
    """Four times the measured error is what the GPU test asserts; that bound must stay below 1e-13 -- a log(1 + z), a float-precision
    logarithm or a softplus that returns 0 below -37 all miss it by orders of magnitude."""
    rec = golden_errors()["objective_max_error"]
    assert sorted(rec) == ["attraction_option_10", "attraction_option_5", "repulsion_option_5"]
    assert all(0 <= v and 4 * v < 1e-13 for v in rec.values()), rec


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
# "quarter_wave", "rows_in_flight"; D = 3 and 101 run the generic kernel whatever the two say: one run each
STEP_CASES = [key + params for key in STEP_KEYS for params in ([(1, 0), (1, 4), (1, 8), (0, 0)] if key[1] in DIMS else [(1, 0)])]


@gpu
@pytest.mark.parametrize("option,D,bs,quarter,inflight", STEP_CASES)
def test_minibatch_steps_on_planted_rows(option, D, bs, quarter, inflight):
    """(a) f2v_minibatch_step against oracle.minibatch after EVERY minibatch, and the rows the rules decide against the rules.  A
    minibatch's rows are read where they are staged (f2v_stage_read: no flush), so that the next step finds them staged still -- its
    sample `lo - 1` and every neighbour of the previous minibatch come from the second matrix, as in test_minibatch_steps_bit_exact --
    and the whole matrix is read once, at the end."""
    rowptr, colids = graph()
    for nonfinite, epochs in passes_of(option):
        ref = oracle_steps(option, D, bs, nonfinite, epochs)
        conditions(ref["states"][-1], ref["classes"], option, nonfinite)
        eng = F.Engine(rowptr, colids, D)
        try:
            eng.set_param("hub_chunk", CHUNK)
            eng.set_param("quarter_wave", quarter)
            eng.set_param("rows_in_flight", inflight)
            eng.set_embeddings(ref["X0"])
            for k, (lo, hi, ids) in enumerate(ref["plan"]):
                if option == 7 and k % ref["per_epoch"] == 0:
                    eng.set_walks(ref["walks"][k // ref["per_epoch"]])
                eng.minibatch_step(option, lo, hi, ids, NS, LR, bs)
                got = eng.stage_read(lo, hi)
                ok(got, ref["states"][k][lo:hi], ref["classes"], rows=np.arange(lo, hi), what="nonfinite %d, minibatch %d [%d, %d)" % (nonfinite, k, lo, hi))
                for kk, p, want in ref["checks"]:
                    if kk == k:
                        ok(got[p - lo], want, ref["classes"], rows=[p], what="minibatch %d, row %d by the rules" % (k, p))
            ok(eng.get_embeddings(), ref["states"][-1], ref["classes"], what="nonfinite %d, the matrix after the last minibatch" % nonfinite)
        finally:
            eng.close()


def need_round_robin_dispatch():
    """(test_gpu_parity._need_round_robin_dispatch: the chained forms exist only where the dispatch probe saw 8 XCDs round robin)"""
    eng = F.Engine(np.array([0, 1, 2, 2, 2], dtype=np.uint32), np.array([1, 0], dtype=np.uint32), 32)
    good = eng.get_param("xcc_round_robin") == 1
    eng.close()
    if not good:
        pytest.skip("dispatch probe: no 8-XCD round robin on this device; chained launches are off")


# name -> (chain_batches, chain_wide, merge_finalize, wide_epochs, last_train_form)
FORMS = {"one launch each": (0, 0, 1, 1, 0), "one launch each and per tree level": (0, 0, 0, 1, 0), "chained": (1, 0, 1, 1, 1), "wide": (1, 1, 1, 1, 2),
         "wide, epochs chained": (1, 1, 1, 2, 2)}


@gpu
@pytest.mark.parametrize("option,D,fanin", TRAIN_KEYS)
def test_train_forms_on_planted_rows(option, D, fanin):
    """(b) every launch form of f2v_train from the planted matrix, against oracle.train and so against one another."""
    need_round_robin_dispatch()
    rowptr, colids = graph()
    X0, classes, want, epochs, nonfinite = oracle_train(option, D, fanin)
    conditions(want, classes, option, nonfinite, small=option != 5)
    for name, (chain, wide, merge, wide_epochs, form) in FORMS.items():
        if option == 7 and wide:
            continue  # (the walk options run one launch each, or chained)
        if D not in DIMS:
            form = 0      # (the generic kernel: every request falls back to one launch per minibatch)
        eng = F.Engine(rowptr, colids, D)
        try:
            for key, v in (("hub_chunk", CHUNK), ("hub_fanin", fanin), ("merge_finalize", merge), ("chain_batches", chain), ("chain_wide", wide),
                           ("wide_epochs", wide_epochs)):
                eng.set_param(key, v)
            eng.set_embeddings(X0)
            eng.srand(1)
            eng.train(option, epochs, BATCH)
            if D % 32 == 0 or form != 1:  # (rows narrower than a line chain only in the wide form)
                assert eng.get_param("last_train_form") == form, name
            if form == 2:  # (a launch carries several epochs only where no row needs combine-tree nodes: at most fanin^2 pieces)
                assert (eng.get_param("last_wide_epochs") > 1) == (wide_epochs > 1 and fanin == 32), name
            ok(eng.get_embeddings(), want, classes, what=name)
        finally:
            eng.close()


EXACT_CASES = [(D, qmin, rows, epochs) for D in DIMS for qmin in (0, 1 << 20) for rows in (4, 16) for epochs in (1, 2)]
EXACT_CASES += [(D, 1 << 20, rows, epochs) for D in (3, 101) for rows in (4, 16) for epochs in (1, 2)]


@gpu
@pytest.mark.parametrize("D,qmin,rows,epochs", EXACT_CASES)
def test_exact_training_on_planted_rows(D, qmin, rows, epochs):
    """(c) option 1 against exact_ref in the engine's order: both pair-kernel layouts, one and four rows per wavefront / wavefronts per
    workgroup."""
    X0, classes, want = exact_restated(N, D, epochs)
    conditions(want, classes, 1, True)
    eng = F.Engine(*graph(), D)
    try:
        eng.set_param("exact_quarter_min", qmin)
        eng.set_param("exact_rows", rows)
        eng.set_embeddings(X0)
        eng.train(1, epochs, BATCH)
        assert eng.get_param("last_exact_quarter") == int(qmin == 0 and D % 4 == 0) and eng.get_param("last_exact_rows") == rows
        ok(eng.get_embeddings(), want, classes)
    finally:
        eng.close()


@gpu
def test_exact_training_with_a_planted_row_beyond_the_first_span():
    X0, classes, want = exact_restated(1100, 128, 1)
    conditions(want, classes, 1, True)
    eng = F.Engine(*graph(1100), 128)
    try:
        eng.set_embeddings(X0)
        eng.train(1, 1, 384)
        ok(eng.get_embeddings(), want, classes)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("math,D,iters,ns", FOLD_KEYS)
def test_fold_in_on_planted_rows(math, D, iters, ns):
    """(d) f2v_fold_in against foldin_ref: lists that name every planted class, from the neighbours' mean and from a given start that
    holds a duplicate of a resident row."""
    for init in ("mean", "given"):
        resident, classes, lists, given, want = fold_restated(math, D, iters, ns, init)
        eng = F.Engine(*graph(), D)
        try:
            eng.set_embeddings(resident)
            got = eng.fold_in(lists, option=math, iters=iters, ns=ns, lr=LR, init="mean" if given is None else given)
        finally:
            eng.close()
        assert E.same_values(got, want), "init %s: %s (rows are new vertices: lists of %s)" % (init, E.difference(got, want), [len(l) for l in lists])


def objective_errors():
    """The device's objective on the two-vertex graph with the single nonzero (0, 1), one z at a time -> the largest error per term over
    the finite cases; the kinds (finite, inf, NaN) are asserted on the way."""
    rowptr, colids = two_vertices(True)
    eng = F.Engine(rowptr, colids, OBJ_D)
    worst = {"attraction_option_5": 0.0, "attraction_option_10": 0.0, "repulsion_option_5": 0.0}
    try:
        for option, zs, sigmoid in ((5, Z5, False), (10, Z10, True)):
            for z in zs:
                eng.set_embeddings(pair_matrix(z, sigmoid))
                att5, att10, rep5, unit = ref_terms(z, precise=have_mpmath())
                got = eng.objective(option, 0)
                assert (got.positive_pairs, got.negative_pairs, got.repulsion) == (1, 0, 0.0)
                want = att10 if sigmoid else att5
                assert kind(got.attraction) == kind(want), (option, z, got.attraction)
                if kind(want) == "finite":
                    err = error_of(got.attraction, want)
                    print("option %d z = %r: attraction %r, error %.3g" % (option, z, got.attraction, err))
                    worst["attraction_option_%d" % option] = max(worst["attraction_option_%d" % option], err)
                if not sigmoid:
                    got = eng.objective(option, 1)  # every sample is vertex 0: the self term and the (1, 0) term
                    assert (got.positive_pairs, got.negative_pairs) == (1, 2)
                    assert kind(got.repulsion) == kind(rep5), (z, got.repulsion)
                    if kind(rep5) == "finite":
                        err = error_of(got.repulsion, rep5, unit)
                        print("option 5 z = %r: repulsion %r, error %.3g of its unit" % (z, got.repulsion, err))
                        worst["repulsion_option_5"] = max(worst["repulsion_option_5"], err)
    finally:
        eng.close()
    return worst


@gpu
def test_objective_terms_one_pair_at_a_time():
    """(e) log1p(z), softplus(-z) and the cancelling repulsion of the device against 50 digits: four times the recorded error at the
    most (tests/golden/extreme_values.json, written from a measured run), which test_recorded_objective_errors_... keeps below 1e-13."""
    rec = golden_errors()["objective_max_error"]
    worst = objective_errors()
    print("measured:", json.dumps(worst))
    for key, v in worst.items():
        assert v <= 4 * rec[key], (key, v, rec[key])
