"""TEST INFRASTRUCTURE: what the floating-point analysers (nearest neighbours, the index, k-means, silhouette and Davies-Bouldin, PCA,
trustworthiness, t-SNE, the logistic-regression features) are given by tests/test_analysis_values.py, and their special-value rules
stated by hand a second time (DESIGN.md "Special values in the analysers").  No GPU here.

graph / matrix / vector_queries   a ring of 300 vertices with chords; the four matrices `finite`, `nonfinite` (extreme_values.planted),
                                  `tiny` (uniform x 1e-19: every product and square is subnormal or zero) and `huge` (uniform x 1e18:
                                  chains end near FLT_MAX); queries that are no rows of the matrix
labelling / given_index / ...     the labellings of the separation cases, the caller-given index, the k-means start, the t-SNE start
same_bits                         extreme_values.same_values for any float width: a NaN where a NaN is expected, identical bits elsewhere
expected_score / check_order      one nearest-neighbour score and the ranking BY RULE (include/f2v.h), never through nearest_ref:
                                  NotSpecial for a pair whose score the rules alone do not decide
expected_s / expected_r           s(i) from a(i), b(i) and R_cd from the scatters and the centroid distance, by rule
expected_tsne_pair                w and r of a t-SNE pair where a = 0 or a = inf"""
import functools

import numpy as np

import extreme_values as E
from extreme_values import NotSpecial

F32, F64 = np.float32, np.float64
FLT_MAX = E.FLT_MAX
N = 300                      # three candidate tiles of 128, the last with 44 live rows
DIMS = (16, 100, 128, 200)   # below a chunk of 32 dimensions; no multiple of it; the 128-query block; the 32-query block
MATRICES = ("finite", "nonfinite", "tiny", "huge")
METRICS = ("dot", "l2", "cos")
# The seed of a planted matrix by D: those of tests/test_extreme_values.py (SEEDS there), so that the analysers see the very start
# matrices the force kernels are run on.  No condition of tests/test_analysis_values.py needed another choice: with them the first
# 128 of the `finite` results hold subnormal dot and L2 scores at every D (0.7 % and 0.1 % at D = 16), `nonfinite` returns 0.7 - 1.3 %
# NaN and 1 - 1.7 % infinite scores, and the squared norm of a "3e18" row overflows from D = 100 on (9e36 x the sum of D squares of
# uniform numbers: 4.8e37 at D = 16, 3e38 and more from D = 100) -- at D = 16 the only overflowing norm is that of the "1e19" row.
SEEDS = {16: 20, 100: 4}
SMALLEST = 2.0 ** -149       # the smallest fp32 subnormal; a product below half of it rounds to a zero


def seed_of(D):
    return SEEDS.get(D, 5)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(n=N):
    """A ring (tests/test_logreg.ring) plus the chords v -- v + 37 for every tenth v: symmetric, ascending inside a row."""
    lists = [{(v - 1) % n, (v + 1) % n} for v in range(n)]
    for v in range(0, n, 10):
        lists[v].add((v + 37) % n)
        lists[(v + 37) % n].add(v)
    rowptr = np.zeros(n + 1, dtype=np.uint32)
    rowptr[1:] = np.cumsum([len(l) for l in lists])
    colids = np.array([j for l in lists for j in sorted(l)], dtype=np.uint32)
    rowptr.setflags(write=False)
    colids.setflags(write=False)
    return rowptr, colids


@functools.lru_cache(maxsize=None)
def matrix(name, D, n=N):
    """-> (X float32 [n, D] read-only, classes: name -> rows).  `finite` / `nonfinite`: extreme_values.planted; `inf_only`: nonfinite
    with the two NaN classes left unplanted (k-means); `nan_column`: nonfinite without the all-NaN row (the PCA mean); `tiny`, `huge`:
    whole-matrix scales, no classes."""
    with np.errstate(all="ignore"):
        if name in ("finite", "nonfinite"):
            X, classes = E.planted(n, D, seed_of(D), name == "nonfinite")
        elif name in ("inf_only", "nan_column"):
            X, classes = E.planted(n, D, seed_of(D), True)
            plain = E.planted(n, D, seed_of(D), False)[0]
            for cls in ("nan_row", "nan_one") if name == "inf_only" else ("nan_row",):
                for r in classes.pop(cls):
                    X[r] = plain[r]
        elif name in ("tiny", "huge"):
            X = (np.random.default_rng(seed_of(D) + 100).uniform(-1, 1, (n, D)).astype(F32) * F32(1e-19 if name == "tiny" else 1e18)).astype(F32)
            classes = {}
        else:
            raise KeyError(name)
    X.setflags(write=False)
    return X, classes


def planted_rows(classes):
    return sorted(r for rows in classes.values() for r in rows)


@functools.lru_cache(maxsize=None)
def vector_queries(D):
    """Queries that are no rows: a zero vector, a -0 vector, a 1e-40 vector, FLT_MAX in one component, a NaN in one component."""
    rng = np.random.default_rng(900 + D)
    Q = rng.uniform(-1, 1, (5, D)).astype(F32)
    Q[0] = F32(0.0)
    Q[1] = F32(-0.0)
    Q[2] = np.where(Q[2] < 0, F32(-1e-40), F32(1e-40))
    Q[3, min(2, D - 1)] = F32(FLT_MAX)
    Q[4, min(3, D - 1)] = np.nan
    Q.setflags(write=False)
    return Q


QUERY_NAMES = ("zero", "negzero", "1e-40", "FLT_MAX", "nan_one")


def few_queries(classes, n=N):
    """20 query rows (the 32-query form at every D): planted rows of every class first, ordinary rows after them."""
    q = [rows[0] for rows in classes.values()][:14]
    q += [r for r in range(3, n, 29) if r not in q][:20 - len(q)]
    return np.array(q, dtype=np.uint32)


def labelling(which, classes, n=N):
    """The labellings of the separation cases (a) .. (c): `a` every fourth vertex; `b` the planted rows alone in cluster 0, the rest in
    1 .. 4; `c` the planted rows in cluster 4, the rest in 0 .. 3."""
    v = np.arange(n)
    if which == "a":
        return (v % 4).astype(np.uint32)
    lab = (v % 4 + (1 if which == "b" else 0)).astype(np.uint32)
    lab[planted_rows(classes)] = 0 if which == "b" else 4
    return lab


@functools.lru_cache(maxsize=None)
def coincident_case(D, n=N):
    """Case (d) -> (X, labels, rows dict).  `finite` with the two "equal" rows made multiples of 2^-10 (still equal), a third copy of them
    at row 1, and rows 2 and 3 set to that row +- 0.25 (exact).  Cluster 0 = the equal rows (scatter 0, a(i) = 0), cluster 1 = rows 2, 3
    (the same centroid, scatter > 0), cluster 2 = row 1 alone (the same centroid, scatter 0), the rest in clusters 3 and 4."""
    X = matrix("finite", D, n)[0].copy()
    classes = matrix("finite", D, n)[1]
    a, b = classes["equal"]
    coarse = (np.round(X[a].astype(F64) * 1024.0) / 1024.0).astype(F32)
    X[a] = X[b] = X[1] = coarse
    X[2], X[3] = coarse + F32(0.25), coarse - F32(0.25)
    assert np.array_equal((X[2].astype(F64) + X[3].astype(F64)) / 2.0, coarse.astype(F64))
    lab = (3 + np.arange(n) % 2).astype(np.uint32)
    lab[[a, b]], lab[[2, 3]], lab[1] = 0, 1, 2
    X.setflags(write=False)
    return X, lab, dict(equal=(a, b), spread=(2, 3), single=1)


def kmeans_init(X):
    """Five ordinary rows (no planted row lies below row 7)."""
    return np.ascontiguousarray(X[[0, 1, 2, 3, 4]])


@functools.lru_cache(maxsize=None)
def given_index(D, n=N):
    """-> (labels arange % 5, centroids [5, D]).  Lists 1 and 2 have the centroids +u x 1e-30 and -u x 1e-30: their squares underflow, so
    their cosine r is 0 and their cosine scores are the zeros +0 / -0 by the sign of the dot product -- one score, ranked by list index."""
    rng = np.random.default_rng(700 + D)
    C = rng.uniform(-1, 1, (5, D)).astype(F32)
    u = rng.uniform(0.5, 1, D).astype(F32)
    C[1], C[2] = u * F32(1e-30), -(u * F32(1e-30))
    C.setflags(write=False)
    return (np.arange(n) % 5).astype(np.uint32), C


@functools.lru_cache(maxsize=None)
def tsne_points(m=128, D=8):
    """A benign matrix for P: N(0, 1), with rows 1, 3 and 7 close to rows 0, 2 and 6, so that the coincident pair, the pair whose squares
    underflow and the pair with a = inf are nonzeros of P (attraction and KL evaluate them, not the repulsion alone)."""
    rng = np.random.default_rng(100 + m)
    X = rng.standard_normal((m, D)).astype(F32)
    for i in (0, 2, 6):
        X[i + 1] = X[i] + F32(0.01) * rng.standard_normal(D).astype(F32)
    X.setflags(write=False)
    return X


TSNE_SPECIAL = dict(coincident=(0, 1), underflow=(2, 3), small=4, negzero=5, far=(6, 7))


def tsne_start(m, d2):
    """1e-4 x N(0, 1) with: points 0, 1 coincident; 2, 3 1e-24 apart (the square underflows: a = 0); 4 at (1e-30, -1e-30); 5 at
    (-0, +0); 6 at (1e19, 0) and 7 at (-1e19, 1e19): a = 4e38 + 1e38 is inf in fp32, so w = 0 while t is finite."""
    y = 1e-4 * np.random.default_rng(7 * m + d2).standard_normal((m, d2))
    y[1] = y[0]
    y[2:8] = 0.0
    y[2, 0], y[3, 0] = 1e-24, 2e-24
    y[4, :2] = 1e-30, -1e-30
    y[5, 0] = -0.0
    y[6, 0] = 1e19
    y[7, :2] = -1e19, 1e19
    return y


def logreg_weights(D, classes=3):
    W = np.random.default_rng(300 + D).standard_normal((classes, D + 1))
    W[1, : D // 2] = 0.0   # zero weights: inf x 0 in the chain
    W[2, -1] = 0.0         # no bias: a chain of subnormal features is the whole decision value
    return W


def logreg_pairs(classes, n=N, m=120):
    """Pairs that put every planted class on either side, and a == b."""
    rng = np.random.default_rng(11)
    pl = planted_rows(classes) if classes else list(range(7, 263, 8))
    a = np.array([pl[i % len(pl)] for i in range(m)], dtype=np.uint32)
    b = rng.integers(0, n, m).astype(np.uint32)
    b[::3] = [pl[(5 * i + 1) % len(pl)] for i in range(len(b[::3]))]
    b[1::10] = a[1::10]
    return a, b


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def same_bits(got, want):
    """extreme_values.same_values for fp32 AND fp64 results: equal shapes and widths, a NaN at the same positions, identical bits
    everywhere else (the sign of a zero and of an inf included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape or got.dtype not in (np.dtype(F32), np.dtype(F64)):
        return False
    if got.dtype == np.dtype(F32):
        return E.same_values(got, want)
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]))


def no_negative_zero(scores):
    s = np.asarray(scores)
    return not (np.signbit(s) & (s == 0)).any()


# ---- nearest neighbours by rule ------------------------------------------------------------------------------------------------------
def _sure_overflow(total):
    """Does a chain of non-negative terms whose exact sum is `total` overflow?  The chain's roundings move it by less than 1e-4 of
    itself (D <= 200 roundings of 2^-24 each): surely above -> True, surely below -> False, in between NotSpecial."""
    if total > FLT_MAX * (1 + 1e-4):
        return True
    if total < FLT_MAX * (1 - 1e-4):
        return False
    raise NotSpecial("the chain may or may not overflow")


def squared_norm_class(v):
    """'nan' | 'inf' | 'zero' | 'number': the class of chain_d fma(v_d, v_d, acc) by rule."""
    v = np.asarray(v, dtype=F32)
    if np.isnan(v).any():
        return "nan"
    if np.isinf(v).any():
        return "inf"
    sq = v.astype(F64) ** 2
    if _sure_overflow(float(sq.sum())):
        return "inf"
    if (sq <= SMALLEST / 2).all():  # every square rounds to +0 on a +0 accumulator
        return "zero"
    return "number"


def dot_class(q, c):
    """-> ('nan' | '+inf' | '-inf' | 'zero' | 'pzero' | 'exact' | 'finite', value): the class of the dot chain by rule.  'pzero': every
    product is an exact zero, so the accumulator never leaves +0 (+0 + -0 = +0); 'zero': every product is below half the smallest
    subnormal, the score is a zero of either sign; 'exact': one product is not zero, the score is that product rounded once."""
    q, c = np.asarray(q, dtype=F32), np.asarray(c, dtype=F32)
    with np.errstate(all="ignore"):
        p = q.astype(F64) * c.astype(F64)  # exact (or inf / NaN as in fp32)
    if np.isnan(p).any() or ((p == np.inf).any() and (p == -np.inf).any()):
        return "nan", None
    inf = np.isinf(p)
    mag = float(np.abs(p[~inf]).sum())
    if inf.any():
        if mag >= FLT_MAX / 2:
            raise NotSpecial("an infinite product among sums that may overflow the other way")
        return ("+inf" if p[inf][0] > 0 else "-inf"), None
    nz = np.flatnonzero(p)
    if not len(nz):
        return "pzero", F32(0.0)
    if (np.abs(p) <= SMALLEST / 2).all():
        return "zero", F32(0.0)
    if len(nz) == 1:
        with np.errstate(all="ignore"):
            return "exact", F32(p[nz[0]])
    if mag < FLT_MAX / 2:
        return "finite", None
    raise NotSpecial("a dot product whose partial sums may overflow")


def expected_score(metric, q, c):
    """The score of (query q, row c) where the rules of include/f2v.h decide it -> float32 (a NaN, an inf, a zero -- returned as +0, the
    sign the call reports -- or the one rounded product); NotSpecial otherwise."""
    q, c = np.asarray(q, dtype=F32), np.asarray(c, dtype=F32)
    if metric == "l2":
        with np.errstate(all="ignore"):
            t = q - c
        if np.isnan(t).any():
            return F32(np.nan)
        if np.isinf(t).any():
            return F32(-np.inf)
        sq = t.astype(F64) ** 2
        if _sure_overflow(float(sq.sum())):
            return F32(-np.inf)
        if (sq <= SMALLEST / 2).all():  # equal rows, or differences whose squares all underflow: -(+0), reported as +0
            return F32(0.0)
        raise NotSpecial("an ordinary distance")
    kind, value = dot_class(q, c)
    if metric == "dot":
        if kind == "nan":
            return F32(np.nan)
        if kind in ("+inf", "-inf"):
            return F32(np.inf if kind == "+inf" else -np.inf)
        if kind in ("pzero", "zero", "exact"):
            return value
        raise NotSpecial("an ordinary dot product")
    nq, nc = squared_norm_class(q), squared_norm_class(c)
    if kind == "nan" or "nan" in (nq, nc):
        return F32(np.nan)
    infinite = kind in ("+inf", "-inf")
    if nq in ("zero", "inf"):          # r_q = 0: dot x 0 first, then x r_c, which is finite (at most 2^74.5) or 0
        return F32(np.nan) if infinite else F32(0.0)
    if nc in ("zero", "inf"):          # r_c = 0 meets x = dot x r_q
        if infinite:
            return F32(np.nan)
        if kind in ("pzero", "zero"):
            return F32(0.0)
        sq = float((q.astype(F64) ** 2).sum()) * (1 - 1e-4)
        mag = float(np.abs(q.astype(F64) * c.astype(F64)).sum())
        if sq > 0 and mag / np.sqrt(sq) < FLT_MAX / 2:  # x cannot have overflowed
            return F32(0.0)
        raise NotSpecial("dot x r_q may overflow before it meets r_c = 0")
    if kind in ("pzero", "zero"):
        return F32(0.0)
    if infinite:
        return F32(np.inf if kind == "+inf" else -np.inf)
    raise NotSpecial("an ordinary cosine")


def check_order(ids, scores, candidates):
    """The ranking of one query by rule: the result holds min(k, candidates) distinct candidates (all of them where k suffices), a
    number before a NaN, numbers descending with -0 = +0, equal scores and NaNs by ascending id, then padding (0xFFFFFFFF, -inf) ->
    None or the first violation."""
    ids, scores = np.asarray(ids), np.asarray(scores, dtype=F32)
    candidates = set(int(c) for c in candidates)
    count = min(len(ids), len(candidates))
    got, s = ids[:count].tolist(), scores[:count]
    if not (np.all(ids[count:] == 0xFFFFFFFF) and np.all(np.isneginf(scores[count:]))):
        return "the tail is not padding"
    if len(set(got)) != count or not set(got) <= candidates:
        return "not %d distinct candidates" % count
    for x in range(count - 1):
        a, b = s[x], s[x + 1]
        if np.isnan(a):
            if not (np.isnan(b) and got[x] < got[x + 1]):
                return "place %d: a NaN (id %d) before %r (id %d)" % (x, got[x], float(b), got[x + 1])
        elif not (np.isnan(b) or a > b or (a == b and got[x] < got[x + 1])):
            return "place %d: %r (id %d) before %r (id %d)" % (x, float(a), got[x], float(b), got[x + 1])
    return None


# ---- separation by rule --------------------------------------------------------------------------------------------------------------
def expected_s(a, b, own_count):
    """s(i) from a(i), b(i): 0 for a cluster of one; a NaN where either is a NaN (b - a, or the division by a NaN maximum); a NaN where
    either is infinite ((b - inf) / inf, (inf - a) / inf); 0 where a = 0 = b; (b - a) / max(a, b) otherwise."""
    if own_count == 1:
        return 0.0
    if np.isnan(a) or np.isnan(b) or np.isinf(a) or np.isinf(b):
        return float("nan")
    if a == 0.0 and b == 0.0:
        return 0.0
    return (b - a) / max(a, b)


def expected_b(means):
    """b(i) and its cluster from the other clusters' mean distances in ascending cluster order [(c, mean)]: the first candidate, replaced
    only where a later mean is SMALLER -- a NaN mean in front stays, a NaN mean later never enters."""
    best, at = means[0][1], means[0][0]
    for c, m in means[1:]:
        if not np.isnan(m) and not np.isnan(best) and m < best:
            best, at = m, c
    return best, at


def expected_r(sc, sd, m):
    """R_cd of Davies-Bouldin: 0 where S_c + S_d == 0, whatever the distance; (S_c + S_d) / M_cd otherwise -- +inf for coincident
    centroids."""
    if sc + sd == 0.0:
        return 0.0
    if m == 0.0:
        return float("inf")
    return (sc + sd) / m


# ---- t-SNE by rule ---------------------------------------------------------------------------------------------------------------------
def expected_tsne_pair(yi, yj):
    """(w, r [d2]) of pair(i, j) where a is 0 or inf by rule: coincident points, or differences whose squares all underflow, give a = 0,
    w = 1 and r = t (zeros for coincident points); a sum of squares beyond FLT_MAX gives a = inf, w = 1 / inf = 0 and r = (0 x 0) x t =
    a zero of t's sign while t is finite -- never a NaN.  NotSpecial otherwise."""
    yi, yj = np.asarray(yi, dtype=F32), np.asarray(yj, dtype=F32)
    with np.errstate(all="ignore"):
        t = yi - yj
    if not np.isfinite(t).all():
        raise NotSpecial("a difference that is not finite")
    sq = t.astype(F64) ** 2
    if (sq <= SMALLEST / 2).all():
        return F32(1.0), t
    if sq.max() > FLT_MAX * (1 + 1e-6):
        return F32(0.0), np.copysign(F32(0.0), t).astype(F32)
    raise NotSpecial("an ordinary pair")
