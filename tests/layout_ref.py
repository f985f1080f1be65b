"""numpy restatement of the layout definition of include/f2v.h (tests/test_layout.py, tools/): the principal components of a matrix
(fp64 sums in pieces of 4096 vertices taken in order, the scatter matrix as fma chains, the cyclic Jacobi method, order and sign, the
projection) and the trustworthiness / continuity / overlap of a second matrix (the order of tests/nearest_ref.py around every sample).

numpy has no fused multiply-add.  `fma64` forms the product exactly as two doubles (Veltkamp / Dekker), adds the addend with two
TwoSums and folds the two error terms with a round-to-odd addition, so that the last addition rounds as one rounding of the exact value
would (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008); tests/test_layout.py checks it against exact
rational arithmetic.  Nothing here knows how the kernels tile, stage or count."""
from collections import namedtuple

import numpy as np

import kmeans_ref as K
import nearest_ref as R

PIECE = 4096
MAX_SWEEPS = 64
Pca = namedtuple("Pca", "y components mean variance total_variance sweeps converged scatter eigenvalues")
Trust = namedtuple("Trust", "trustworthiness continuity overlap penalty_x penalty_y hits samples_x samples_y")


def _split(a):
    c = 134217729.0 * a
    h = c - (c - a)
    return h, a - h


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma64(a, b, c, sa=None, sb=None):
    """One correctly rounded fp64 fma of float64 arrays (no overflow, no underflow of the product's error term); sa / sb: the
    operands' splits where the caller has them already."""
    with np.errstate(invalid="ignore", over="ignore"):
        ah, al = _split(a) if sa is None else sa
        bh, bl = _split(b) if sb is None else sb
        uh = a * b
        ul = (((ah * bh - uh) + ah * bl) + al * bh) + al * bl
        th, tl = _two_sum(c, ul)
        vh, vl = _two_sum(uh, th)
        s, e = _two_sum(vl, tl)  # vl + tl rounded to odd
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
        z = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        out = vh + z
        return np.where(np.isfinite(uh), out, uh + c)  # an infinite or NaN product: the plain sum has the fma's value


def mean(X):
    """Pieces of 4096 vertices summed per dimension sequentially from +0, the piece sums added in order, divided by n."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    parts = np.array([K.seq_sum(X64[p:p + PIECE]) for p in range(0, len(X64), PIECE)])
    return K.seq_sum(parts) / float(len(X64))


def scatter(X, m=None):
    """The D x D scatter matrix: per piece the chain fma(z_vd, z_ve, acc) over ascending vertex id for d <= e, pieces added in order."""
    X = np.asarray(X, dtype=np.float32)
    n, D = X.shape
    m = mean(X) if m is None else m
    Z = X.astype(np.float64) - m
    Zh, Zl = _split(Z)
    iu, ju = np.triu_indices(D)
    total = np.zeros(len(iu))
    for p in range(0, n, PIECE):
        acc = np.zeros(len(iu))
        for v in range(p, min(n, p + PIECE)):
            acc = fma64(Z[v, iu], Z[v, ju], acc, (Zh[v, iu], Zl[v, iu]), (Zh[v, ju], Zl[v, ju]))
        total = total + acc
    S = np.zeros((D, D))
    S[iu, ju] = total
    S[ju, iu] = total
    return S


def jacobi(S):
    """The cyclic Jacobi method of f2v.h -> (eigenvalues = the diagonal, V with the eigenvectors as columns, sweeps, converged)."""
    A = np.array(S, dtype=np.float64)
    D = len(A)
    V = np.eye(D)
    sweeps, converged = 0, False
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(MAX_SWEEPS):
            rotated = False
            for p in range(D - 1):
                for q in range(p + 1, D):
                    apq, app, aqq = A[p, q], A[p, p], A[q, q]
                    if apq == 0.0:
                        continue
                    g = abs(apq)
                    if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                        A[p, q] = A[q, p] = 0.0
                        continue
                    theta = (aqq - app) / (2.0 * apq)
                    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    rp, rq = A[p].copy(), A[q].copy()
                    A[p], A[q] = c * rp - s * rq, s * rp + c * rq
                    cp, cq = A[:, p].copy(), A[:, q].copy()
                    A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                    A[p, q] = A[q, p] = 0.0
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
                    rotated = True
            sweeps += 1
            if not rotated:
                converged = True
                break
    return np.diag(A).copy(), V, sweeps, converged


def components(lam, V, d2):
    """Eigenvalue descending, ties by ascending column, NaN last; a component's entry of largest magnitude (the lowest d) is positive."""
    nan = np.isnan(lam)
    order = np.lexsort((np.arange(len(lam)), np.where(nan, 0.0, -lam), nan))[:d2]
    W = V[:, order].T.copy()
    for w in W:
        if w[int(np.argmax(np.abs(w)))] < 0.0:
            w *= -1.0
    return W, lam[order]


def project(X, m, W):
    X = np.asarray(X, dtype=np.float32)
    Z = X.astype(np.float64) - m
    acc = np.zeros((len(X), len(W)))
    for d in range(X.shape[1]):
        acc = fma64(Z[:, d:d + 1], W[None, :, d], acc)
    return acc.astype(np.float32)


def pca(X, d2=2):
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = len(X)
    m = mean(X)
    S = scatter(X, m)
    lam, V, sweeps, converged = jacobi(S)
    W, top = components(lam, V, d2)
    return Pca(project(X, m, W), W, m, top / float(n - 1), float(K.seq_sum(np.diag(S))) / float(n - 1), sweeps, converged, S, lam)


def places(M, ids):
    """[len(ids), n] int64: r_M(i, j), the 1-based place of j in the order of M around i = ids[q]; 0 for j = i."""
    M = np.ascontiguousarray(M, dtype=np.float32)
    n = len(M)
    out = np.zeros((len(ids), n), dtype=np.int64)
    cand = np.arange(n)
    step = max(1, 2000000 // n)
    for lo in range(0, len(ids), step):
        S = R.scores(M[ids[lo:lo + step]], M, "l2")
        for q in range(len(S)):
            s, i = S[q], ids[lo + q]
            nan = np.isnan(s)
            order = np.lexsort((cand, np.where(nan, np.float32(0), -s), nan))
            order = order[order != i]
            out[lo + q, order] = np.arange(1, n)
    return out


def trust(X, Y, k, ids=None):
    n = len(X)
    ids = np.arange(n) if ids is None else np.asarray(ids, dtype=np.int64)
    rx, ry = places(X, ids), places(Y, ids)
    nx, ny = (rx >= 1) & (rx <= k), (ry >= 1) & (ry <= k)
    px = (np.maximum(rx - k, 0) * ny).sum(axis=1).astype(np.uint64)
    py = (np.maximum(ry - k, 0) * nx).sum(axis=1).astype(np.uint64)
    hits = int((nx & ny).sum())
    sx, sy, nq = int(px.sum()), int(py.sum()), len(ids)
    scale = 2.0 / (float(nq) * k * (2.0 * n - 3.0 * k - 1.0))
    return Trust(1.0 - float(sx) * scale, 1.0 - float(sy) * scale, float(hits) / (float(nq) * k), sx, sy, hits, px, py)
