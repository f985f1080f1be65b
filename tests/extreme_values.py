"""TEST INFRASTRUCTURE: inputs at which fp32 and fp64 arithmetic differs between two correct-looking instruction sequences, a
comparison that knows about NaN, and the hand-derived result of one interaction for the special cases.

planted / planted_graph   a uniform(-1, 1) matrix with classes of rows overwritten (equal rows, rows one ulp apart, scales from 1e-40
                          to 1e19, -0.0, one-hot rows whose dot products sit on fast_SM's thresholds and cell boundaries, NaN, inf),
                          and a graph in which those rows are batch rows, CSR neighbours (of ordinary rows and of split hubs) and samples
same_values / difference  bits equal, NaN where NaN (sign and payload of a NaN are not compared: x86's default NaN is negative, the
                          GPU's is not); the message names the first differing (row, dim) and the row's planted class
expected_pair             one interaction by RULE (include/f2v.h; sample/algorithms.cpp:6-10, :608, :622, :766-770, :867, :907), never
                          through oracle/: the cases in which the result follows from a = 0, a = inf, a NaN, an infinite coefficient
                          or a saturated / exactly known sigmoid -- NotSpecial for every other pair
expected_row              a whole row update chained from such interactions (one piece: a row that "hub_chunk" does not split)
"""
import numpy as np

F32 = np.float32
F64 = np.float64
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = float(np.finfo(F32).tiny)
SM_TABLE_SIZE = 2048
SM_BOUND = 6.0
SM_RES = F32(SM_TABLE_SIZE / (2.0 * SM_BOUND))  # SM_RESOLUTION is a float constant (algorithms.h:49)
HUB_CHUNK = 8
BATCH = 64

# class -> number of rows, in planting order.  The first row of "ulp" / "ulp_tiny" is the row the second one copies.
FINITE_CLASSES = (("1e9", 2), ("equal", 2), ("ulp", 2), ("ulp_tiny", 2), ("3e18", 2), ("1e-20", 2), ("1e-40", 2), ("negzero", 1),
                  ("onehot", 5), ("cells", 7))
NONFINITE_CLASSES = (("nan_row", 1), ("nan_one", 1), ("inf_one", 1), ("ninf_last", 1), ("1e19", 1))
CELLS = (1, 1024, 2047)  # the table cells whose lower boundary a pair of "cells" rows straddles


class NotSpecial(Exception):
    """expected_pair: the result of this interaction does not follow from the special-value rules alone"""


# ---- the planted rows ----------------------------------------------------------------------------------------------------------
def class_rows(n):
    """class -> its rows, the same for every D and for nonfinite on or off: one planted row every (n - 16) // 32 rows from row 7 on,
    the finite classes dealt round robin so that every minibatch of 64 rows holds several kinds (n = 256: rows 7 .. 224; n = 1100:
    rows 7 .. 1030, the last one beyond the first span of 1024 columns); never a hub (5, n - 3), the row n - 2 that reads them all,
    nor a row within three of another planted row."""
    names = [name for name, k in FINITE_CLASSES + NONFINITE_CLASSES for _ in range(k)]
    stride = (n - 16) // len(names)
    assert stride >= 4, "n too small for the planted rows"
    # deal: slot s takes the s-th name of an order that interleaves the classes (first rows of every class, then second rows, ...)
    # The non-finite classes come last, in the last minibatch of a pass over 256 rows: one pass of a sigmoid option, in which a row
    # that reads a NaN is NaN, then leaves the minibatches before it alone.  (The positions and the readers below are chosen on the
    # CPU so that the runs the tests compare against keep most rows finite and, for options 6 and 7, most entries below 1e6.)
    order, depth = [], 0
    while len(order) < len(names) - len(NONFINITE_CLASSES):
        for name, k in FINITE_CLASSES:
            if depth < k:
                order.append(name)
        depth += 1
    order += [name for name, _ in NONFINITE_CLASSES]
    rows = {}
    for s, name in enumerate(order):
        rows.setdefault(name, []).append(7 + stride * s)
    return rows


def cell_values():
    """For each cell c of CELLS the two neighbouring fp32 values v- < v+ with fast_SM's index c - 1 and c: the index is
    (int)(((double)v + 6.0) * (double)res) with res = float32(2048 / 12.0), as fast_SM computes it."""
    out = []
    for c in CELLS:
        v = F32((c / F64(SM_RES)) - SM_BOUND)
        idx = lambda x: int((F64(x) + SM_BOUND) * F64(SM_RES))  # noqa: E731
        while idx(v) >= c:
            v = np.nextafter(v, F32(-np.inf))
        while idx(np.nextafter(v, F32(np.inf))) < c:
            v = np.nextafter(v, F32(np.inf))
        hi = np.nextafter(v, F32(np.inf))
        assert idx(v) == c - 1 and idx(hi) == c
        out += [v, hi]
    return out


def planted(n, D, seed, nonfinite):
    """-> (X float32 [n, D], classes: name -> rows).  With nonfinite off the rows of the non-finite classes keep their uniform values
    (and are not named in the dict)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, D)).astype(F32)
    rows = class_rows(n)
    k = min(1, D - 1)  # the dimension a single special component goes to (not the one-hot rows' dimension 0 where D allows)
    with np.errstate(over="ignore", under="ignore"):
        a, b = rows["equal"]
        X[b] = X[a]
        base, moved = rows["ulp"]
        X[moved] = X[base]
        X[moved, k] = np.nextafter(X[base, k], F32(2.0))
        for name, s in (("1e9", 1e9), ("3e18", 3e18), ("1e-20", 1e-20), ("1e-40", 1e-40)):
            for r in rows[name]:
                X[r] = X[r] * F32(s)
        base, moved = rows["ulp_tiny"]  # the same one ulp on a row of magnitude 1e-20: its square underflows to zero
        X[base] = X[base] * F32(1e-20)
        X[moved] = X[base]
        X[moved, k] = np.nextafter(X[base, k], F32(2.0))
        X[rows["negzero"][0]] = F32(-0.0)
        three = F32(3.0)
        for r, v in zip(rows["onehot"], (F32(2.0), three, np.nextafter(three, F32(4.0)), np.nextafter(three, F32(2.0)), F32(-3.0))):
            X[r] = 0.0
            X[r, 0] = v
        for r, v in zip(rows["cells"], [F32(1.0)] + cell_values()):
            X[r] = 0.0
            X[r, 0] = v
        classes = {name: list(rows[name]) for name, _ in FINITE_CLASSES}
        if nonfinite:
            X[rows["nan_row"][0]] = np.nan
            X[rows["nan_one"][0], k] = np.nan
            X[rows["inf_one"][0], k] = np.inf
            X[rows["ninf_last"][0], D - 1] = -np.inf
            X[rows["1e19"][0]] = X[rows["1e19"][0]] * F32(1e19)
            classes.update({name: list(rows[name]) for name, _ in NONFINITE_CLASSES})
    return X, classes


def class_of(classes, row):
    for name, rows in (classes or {}).items():
        if row in rows:
            return name
    return None


def wild_rows(n):
    """The rows whose readers a sigmoid option turns non-finite or huge: the non-finite classes and the scales 1e9 and 3e18."""
    rows = class_rows(n)
    return sorted(r for name in [c for c, _ in NONFINITE_CLASSES] + ["1e9", "3e18"] for r in rows[name])


def planted_graph(n, seed=3):
    """random_graph's recipe (average degree 6, hubs of 40 and 90 at rows 5 and n - 3), then: every planted row p becomes a neighbour
    of the ordinary row p + 3 and of row n - 2, which reads all 32 of them, is split into pieces by "hub_chunk" 8 and is read by
    nobody; the planted rows that are not wild (wild_rows) also of both hubs.  A wild row has no other reader besides its partners: a
    sigmoid option hands its size or its NaN on to every reader.  A planted row's own list is its class partners (the other rows of
    its class; the first "onehot" / "cells" row and the others name each other; a few pairs across classes), row p + 2 and its random
    neighbours, cut to 8 entries so that the row stays one piece.  Ascending inside a row; not symmetric."""
    from test_gpu_parity import random_graph
    rowptr, colids = random_graph(n, 6, seed, hubs=((5, 40), (n - 3, 90)))
    lists = [list(colids[rowptr[i]:rowptr[i + 1]]) for i in range(n)]
    rows = class_rows(n)
    partners = {}
    for name, rs in rows.items():
        for r in rs:
            partners[r] = [q for q in rs if q != r] if name not in ("onehot", "cells") else ([q for q in rs[1:]] if r == rs[0] else [rs[0]])
    for x, y in (("negzero", "equal"), ("1e-40", "1e-20"), ("1e9", "3e18"), ("nan_row", "inf_one"), ("nan_one", "ninf_last"), ("1e19", "1e9"),
                 ("inf_one", "ninf_last"), ("onehot", "cells"), ("ulp_tiny", "1e-40")):
        partners[rows[x][0]].append(rows[y][0])
        partners[rows[y][0]].append(rows[x][0])
    wild, sink = wild_rows(n), n - 2
    lists = [[j for j in l if j not in wild and j != sink] for l in lists]  # (a wild row has the readers named below and no others)
    for p, mates in partners.items():
        own = []
        for j in mates + [p + 2] + lists[p]:
            if j not in own and j != p:
                own.append(int(j))
        lists[p] = own[:HUB_CHUNK]
        for reader in ((p + 3, sink) if p in wild else (p + 3, sink, 5, n - 3)):
            lists[reader].append(p)
    lists = [sorted(l) for l in lists]
    rowptr = np.zeros(n + 1, dtype=np.uint32)
    rowptr[1:] = np.cumsum([len(l) for l in lists])
    return rowptr, np.array([j for l in lists for j in l], dtype=np.uint32)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _differ(got, want):
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | (~gn & ~wn & (_bits(got) != _bits(want)))


def same_values(got, want):
    """A NaN at the same positions and identical bits everywhere else, the sign of zero and of inf included."""
    return not _differ(got, want).any()


def difference(got, want, classes=None, rows=None):
    """The failure message of same_values: the first differing (row, dim), both bit patterns, the row's planted class.  `rows`: the
    vertex ids of the rows of `got` where they are not 0, 1, ..."""
    bad = np.atleast_2d(_differ(got, want))
    if not bad.any():
        return "same values"
    g, w = np.atleast_2d(np.asarray(got, dtype=F32)), np.atleast_2d(np.asarray(want, dtype=F32))
    r, d = (int(v[0]) for v in np.nonzero(bad))
    row = r if rows is None else int(rows[r])
    name = class_of(classes, row)
    return ("%d values in %d rows differ, first at (row %d, dim %d): got %r (0x%08x), expected %r (0x%08x); the row is %s"
            % (int(bad.sum()), int(bad.any(axis=1).sum()), row, d, float(g[r, d]), int(_bits(g)[r, d]), float(w[r, d]), int(_bits(w)[r, d]),
               "planted: class %r" % name if name else "not a planted row"))


# ---- one interaction by rule -------------------------------------------------------------------------------------------------------
def sm_entry(i):
    """init_SM_TABLE (sample/algorithms.cpp:757-764): x in float, expf, 1.0 / (float) in double, narrowed."""
    x = F32(2.0 * SM_BOUND * i / SM_TABLE_SIZE - SM_BOUND)
    e = F32(np.exp(-F64(x)))  # expf: the correctly rounded value
    return F32(1.0 / F64(F32(1.0) + e))


def sm_table():
    return np.array([sm_entry(i) for i in range(SM_TABLE_SIZE)], dtype=F32)


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        _TABLE = sm_table()
    return _TABLE


def sm_of_exact(v):
    """fast_SM of an exactly known fp32 dot product (sample/algorithms.cpp:766-770; v == 6.0 clamped to the last cell)."""
    if v > F32(SM_BOUND):
        return F32(1.0)
    if v < F32(-SM_BOUND):
        return F32(0.0)
    idx = int((F64(v) + SM_BOUND) * F64(SM_RES))
    return _table()[min(max(idx, 0), SM_TABLE_SIZE - 1)]


def sm_special(xi, xj):
    """The sigmoid factor of the pair where it follows from the rules: a NaN dot product -> table[0]; a dot product beyond +-6 by a
    margin that no summation order can cross -> 1 / 0; a dot product of at most one nonzero term -> exactly known, the table cell."""
    with np.errstate(all="ignore"):
        p = (np.asarray(xi, dtype=F32) * np.asarray(xj, dtype=F32)).astype(F32)
    if np.isnan(p).any() or ((p == np.inf).any() and (p == -np.inf).any()):
        return _table()[0]
    inf = np.isinf(p)
    if inf.any():
        if np.abs(p[~inf].astype(F64)).sum() >= 1e37:  # (a partial sum of the finite terms could overflow the other way)
            raise NotSpecial("an infinite term among large ones")
        return F32(1.0) if p[inf][0] > 0 else F32(0.0)
    nz = np.flatnonzero(p)
    if len(nz) <= 1:
        return sm_of_exact(p[nz[0]] if len(nz) else F32(0.0))
    s, mag = float(p.astype(F64).sum()), float(np.abs(p.astype(F64)).sum())
    if mag >= FLT_MAX / 4:
        raise NotSpecial("a partial sum may overflow")
    if s > SM_BOUND + 1e-5 * mag:
        return F32(1.0)
    if s < -SM_BOUND - 1e-5 * mag:
        return F32(0.0)
    raise NotSpecial("a dot product inside the table's range")


def contribution5(neg, xi, xj, lr):
    """What one interaction of the t-distribution kernel adds to the row's accumulator, by rule (scale() is max then min as compiled:
    NaN -> -5; d1 = 2 / (a (1 + a)) repulsive, -2 / (1 + a) attractive, formed in fp64 and narrowed)."""
    xi, xj, lr = np.asarray(xi, dtype=F32), np.asarray(xj, dtype=F32), F32(lr)
    D = len(xi)
    minus, plus, zero = lr * F32(-5.0), lr * F32(5.0), F32(0.0)
    with np.errstate(all="ignore"):
        diff = xi - xj
        sq = diff * diff
    if np.isnan(diff).any():            # a is NaN, d1 is NaN, every product is NaN: -5 everywhere
        return np.full(D, minus, dtype=F32)
    if np.isinf(diff).any():            # a = inf, d1 = +0 / -0: inf x 0 is NaN -> -5 there; a finite difference x 0 is a zero
        return np.where(np.isinf(diff), minus, zero).astype(F32)
    total = float(sq.astype(F64).sum()) if not np.isinf(sq).any() else np.inf
    if total > 2 * FLT_MAX:             # a overflows from finite differences in every order of summation: d1 = +-0, nothing added
        return np.zeros(D, dtype=F32)
    if total >= FLT_MAX / 2:
        raise NotSpecial("the sum of squares may or may not overflow")
    if not neg:
        if not diff.any():              # a = 0, d1 = -2, every product is -0: the accumulator is unchanged
            return np.zeros(D, dtype=F32)
        raise NotSpecial("an ordinary attraction")
    # below 2^-126 the squares are multiples of 2^-149 and their sum is exact in every order: a is `total`
    if total == 0.0 or (total < FLT_MIN and np.isinf(F32(2.0 / (total * (1.0 + total))))):
        # d1 = +inf (a = 0: 2 / 0): 0 x inf is NaN -> -5; a difference that is not zero x inf -> +-5 by its sign
        return np.where(diff == 0, minus, np.where(diff > 0, plus, minus)).astype(F32)
    nz = np.flatnonzero(diff)
    if len(nz) == 1 and abs(float(diff[nz[0]])) < 1e-3 and total >= FLT_MIN:
        # one difference u, a = u^2 normal: d1 ~ 2 / u^2 is finite, u x d1 ~ 2 / u is beyond the clamp; 0 x d1 = 0 elsewhere
        out = np.zeros(D, dtype=F32)
        out[nz[0]] = plus if diff[nz[0]] > 0 else minus
        return out
    raise NotSpecial("an ordinary repulsion")


def expected_row(option, X, i, nbrs, samples, lr, degree=None):
    """The new row i after its neighbours `nbrs` (attraction) and `samples` (repulsion), in that order, as ONE piece -- every
    interaction by rule; NotSpecial if one of them is none.  Sigmoid options: `degree` is the CSR degree behind degi (option 7: the
    list is the walk), c0 = (double)(lr * degi) with degi = (float)(1.0 / (degree + 1))."""
    X = np.asarray(X, dtype=F32)
    xi, lr = X[i], F32(lr)
    with np.errstate(all="ignore"):
        if option == 5:
            Y = np.zeros(len(xi), dtype=F32)
            for neg, ids in ((False, nbrs), (True, samples)):
                for j in ids:
                    Y = Y + contribution5(neg, xi, X[j], lr)
            return xi + Y
        degi = F32(1.0 / F64((len(nbrs) if degree is None else degree) + 1))
        c0 = F64(lr * degi)
        P = xi.copy()
        for j in nbrs:
            coef = (1.0 - F64(sm_special(xi, X[j]))) * c0                      # algorithms.cpp:867
            P = (X[j].astype(F64) * coef + P.astype(F64)).astype(F32)
        for j in samples:
            w = lr * sm_special(xi, X[j])                                      # algorithms.cpp:907
            P = P - w * X[j]
        return P


def expected_pair(option, neg, xi, xj, lr, c0=None):
    """The row xi after ONE interaction with xj (neg: as a negative sample) where the special-value rules decide it:
    option 5   out = xi + (0 + lr * f): a = 0 / an infinite d1 -> f = -5 where the difference is zero, +-5 by its sign elsewhere
               (repulsion), nothing (attraction); a = inf -> nothing, but -5 where the difference itself is infinite; NaN -> -5 everywhere
    6, 7       sm = 1 beyond +6, 0 beyond -6, table[2047] at 6.0f, table[0] at -6.0f and for a NaN; attraction adds xj * ((1 - sm) * c0)
               in fp64, repulsion subtracts (lr * sm) * xj in fp32
    NotSpecial is raised for every other pair."""
    xi, xj, lr = np.asarray(xi, dtype=F32), np.asarray(xj, dtype=F32), F32(lr)
    with np.errstate(all="ignore"):
        if option == 5:
            return xi + (np.zeros(len(xi), dtype=F32) + contribution5(neg, xi, xj, lr))
        sm = sm_special(xi, xj)
        if not neg:
            return (xj.astype(F64) * ((1.0 - F64(sm)) * F64(c0)) + xi.astype(F64)).astype(F32)
        return xi - (lr * sm) * xj


def c0_of(lr, degree):
    """(double)(lr * degi), degi = (float)(1.0 / (degree + 1)) (sample/algorithms.cpp:854, :867)"""
    return F64(F32(lr) * F32(1.0 / F64(degree + 1)))


def rep_coef(xi, xj):
    """The restated repulsive coefficient (float)(2.0 / (a * (1.0 + a))) of a pair, a the wavefront tree's sum of squares."""
    from exact_ref import pair_sum
    with np.errstate(all="ignore"):
        d = np.asarray(xi, dtype=F32) - np.asarray(xj, dtype=F32)
        a = F64(pair_sum((d * d)[None, :], "engine")[0])
        return F32(2.0 / (a * (1.0 + a)))


def is_subnormal(v):
    return v != 0 and abs(float(v)) < FLT_MIN


# ---- the sample ids of the minibatch-at-a-time runs ---------------------------------------------------------------------------------
def minibatch_plan(n, option, bs, epochs, classes, nonfinite_samples, ns=5, seed=7, batch=BATCH):
    """-> [(lo, hi, ids)] for `epochs` passes.  Shared samples (bs = 0): the row `lo` itself, a row of the previous minibatch (still staged where the caller
    has read nothing but f2v_stage_read in between),
    then for option 5 a NaN row, a row with an inf and one planted finite row (the second "1e9" row in the very first minibatch, whose
    first "1e9" row then meets a subnormal coefficient; after that the classes in turn).  Options 6 / 7 share finite rows only: one
    shared NaN sample would turn the whole minibatch to NaN.  Per-row windows (bs = 1): random rows, with the row itself, a planted
    finite row and -- where nonfinite_samples -- a NaN row and an inf row at fixed places of every window array."""
    rng = np.random.default_rng(seed)
    finite = [r for name, _ in FINITE_CLASSES for r in classes[name]]
    turn = 0
    plan = []
    for _ in range(epochs):
        for lo in range(0, n, batch):
            hi = min(lo + batch, n)
            nid = (hi - lo) + ns - 1 if bs else ns
            ids = rng.integers(0, n - 1, nid).astype(np.uint32)
            if option != 5:  # (the sigmoid options meet a wild row as a sample only where it is put on purpose)
                ids = np.where(np.isin(ids, wild_rows(n)), ids + 3, ids).astype(np.uint32)
            first = not plan
            pick = classes["1e9"][1] if first else finite[(5 * turn) % len(finite)]
            turn += 1
            if not bs:
                ids[0] = lo
                if lo > 0:
                    ids[1] = lo - 1
                if option == 5 and nonfinite_samples:
                    ids[2], ids[3] = classes["nan_row"][0], classes["inf_one"][0]
                ids[4] = pick
            else:
                ids[0] = lo                                    # row lo's own first sample: itself
                ids[classes["1e9"][0] - lo if first else 9] = pick
                if lo > 0:
                    ids[20] = lo - 1
                if nonfinite_samples and (option == 5 or lo >= n // 2):
                    ids[30], ids[41] = classes["nan_row"][0], classes["inf_one"][0]
                    if option == 5:
                        ids[12], ids[50] = classes["nan_one"][0], classes["ninf_last"][0]
            plan.append((lo, hi, ids))
    return plan
