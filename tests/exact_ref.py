"""numpy restatement of the exact all-pairs Force2Vec (option 1), in two orders of summation.

order="reference"  everything sequential, as sample/algorithms.cpp:344-445 runs it: per row one fp32 accumulator over the CSR
                   neighbours, then the columns j < i and j > i ascending; a pair's squared distance summed over d sequentially.
order="engine"     the definition of include/f2v.h: the pair sum is the balanced adjacent-pair tree over next_pow2(D) zero-padded
                   terms, the repulsion is summed in pieces of 64 columns and spans of 16 pieces, the attraction part on its own.

Every operation is one rounded fp32 (or, for the coefficients and the objective, fp64) numpy operation, so both orders are
bit-reproducible; rows are independent inside a minibatch and are computed in chunks on a few threads.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

PIECE = 64
SPAN = 16
F32 = np.float32
_NEG5, _POS5 = F32(-5.0), F32(5.0)


def step_of(epoch):
    """STEP_e: e multiplications by 0.999 from 1.0f, each product formed in fp64 and narrowed."""
    s = F32(1.0)
    for _ in range(int(epoch)):
        s = F32(np.float64(s) * 0.999)
    return s


def scale(v):
    """max(v, -5) then min(., 5) as the reference compiles it: a NaN becomes -5."""
    return np.fmin(np.fmax(v, _NEG5), _POS5)


def pair_sum(sq, order):
    """The sum over the last axis of the rounded squares: sequential, or the adjacent-pair tree over next_pow2(D) terms."""
    if order == "reference":
        return np.add.accumulate(sq, axis=-1, dtype=F32)[..., -1]
    D = sq.shape[-1]
    P = 1
    while P < D:
        P *= 2
    if P != D:
        pad = np.zeros(sq.shape[:-1] + (P,), dtype=F32)
        pad[..., :D] = sq
        sq = pad
    while sq.shape[-1] > 1:
        sq = sq[..., 0::2] + sq[..., 1::2]
    return sq[..., 0]


def _coef_rep(a):
    a = a.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (2.0 / (a * (1.0 + a))).astype(F32)


def _coef_att(a):
    a = a.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (-2.0 / (1.0 + a)).astype(F32)


def _attraction(X, rowptr, colids, rows, step, order, acc):
    """acc[r] += STEP * f over the CSR neighbours of rows[r] in row order (duplicates included), sequentially per row."""
    deg = (rowptr[rows + 1] - rowptr[rows]).astype(np.int64)
    for k in range(int(deg.max()) if len(deg) else 0):
        sel = np.nonzero(deg > k)[0]
        j = colids[rowptr[rows[sel]].astype(np.int64) + k]
        t = X[rows[sel]] - X[j]
        a = pair_sum(t * t, order)
        with np.errstate(invalid="ignore"):
            f = scale(t * _coef_att(a)[:, None]) - scale(t * _coef_rep(a)[:, None])
        acc[sel] = acc[sel] + step * f
    return acc


def _contributions(X, rows, step, order, skip, width):
    """c[r, j] = STEP * scale(t * d1) for every column j < n; `skip` at j == rows[r] and in the columns n .. width-1."""
    n, D = X.shape
    c = np.full((len(rows), width, D), skip, dtype=F32)
    t = X[rows][:, None, :] - X[None, :, :]
    a = pair_sum(t * t, order)
    with np.errstate(invalid="ignore"):
        np.multiply(t, _coef_rep(a)[:, :, None], out=t)
    c[:, :n] = step * scale(t)
    c[np.arange(len(rows)), rows] = skip
    return c


def _rows_update(X, rowptr, colids, rows, step, order):
    n, D = X.shape
    R = len(rows)
    if order == "reference":
        acc = _attraction(X, rowptr, colids, rows, step, order, np.zeros((R, D), dtype=F32))
        # (acc + -0.0 is acc for every acc: a skipped column adds nothing)
        c = _contributions(X, rows, step, order, F32(-0.0), n)
        buf = np.empty((R, n + 1, D), dtype=F32)
        buf[:, 0] = acc
        buf[:, 1:] = c
        return np.add.accumulate(buf, axis=1, dtype=F32)[:, -1]
    A = _attraction(X, rowptr, colids, rows, step, order, np.zeros((R, D), dtype=F32))
    pieces = (n + PIECE - 1) // PIECE
    spans = (pieces + SPAN - 1) // SPAN
    # (sums that start from +0 are never -0, so a skipped column or a piece past the last one may add +0)
    c = _contributions(X, rows, step, order, F32(0.0), pieces * PIECE).reshape(R, pieces, PIECE, D)
    P = np.zeros((R, spans * SPAN, D), dtype=F32)
    for p in range(PIECE):
        P[:, :pieces] = P[:, :pieces] + c[:, :, p]
    P = P.reshape(R, spans, SPAN, D)
    S = np.zeros((R, spans, D), dtype=F32)
    for q in range(SPAN):
        S = S + P[:, :, q]
    Y = A
    for s in range(spans):
        Y = Y + S[:, s]
    return Y


def _threads(threads):
    return threads if threads else max(1, min(8, os.cpu_count() or 1))


def train(X0, rowptr, colids, batch, epochs, first_epoch=0, order="engine", threads=0, chunk=16, special_values=False):
    """`epochs` epochs from epoch index `first_epoch` on; returns the new matrix (X0 is left alone).  special_values: the matrix holds
    rows of 1e19, inf or NaN on purpose -- inf - inf and overflowing squares are part of the definition then, and numpy's warnings
    about them are switched off (here, not by the caller: the worker threads have a floating-point error state of their own)."""
    assert order in ("engine", "reference")
    quiet = dict(over="ignore", invalid="ignore") if special_values else {}

    def update(rows):
        with np.errstate(**quiet):
            return _rows_update(X, rowptr, colids, rows, step, order)

    X = np.array(X0, dtype=F32, copy=True)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colids = np.asarray(colids, dtype=np.int64)
    n = X.shape[0]
    step = step_of(first_epoch)
    with ThreadPoolExecutor(_threads(threads)) as pool:
        for _ in range(epochs):
            for lo in range(0, n, batch):
                hi = min(lo + batch, n)
                groups = [np.arange(g, min(g + chunk, hi)) for g in range(lo, hi, chunk)]
                Y = list(pool.map(update, groups))
                with np.errstate(**quiet):
                    X[lo:hi] = X[lo:hi] + np.concatenate(Y)  # every read above saw the matrix as it was before the minibatch
            step = F32(np.float64(step) * 0.999)
    return X


# ---- the exact objective ---------------------------------------------------------------------------------------------------------
def flog(x):
    """flog of include/f2v.h: log of positive normal fp64 numbers from +, * and one division in a stated order."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    k = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    dk = (k + big).astype(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01))
    t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)))
    R = t2 + t1
    hfsq = (0.5 * f) * f
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f)


def _chain(terms, width):
    """terms [rows, k * width] -> per row: pieces of `width` summed sequentially from +0, the piece sums sequentially from +0."""
    rows = terms.shape[0]
    t = terms.reshape(rows, -1, width)
    piece = np.zeros(t.shape[:2])
    for p in range(width):
        piece = piece + t[:, :, p]
    out = np.zeros(rows)
    for k in range(piece.shape[1]):
        out = out + piece[:, k]
    return out


def objective(X, rowptr, colids, chunk=64):
    """(loss, attraction, repulsion, positive_pairs, negative_pairs) of the definition, bit for bit."""
    X = np.asarray(X, dtype=F32)
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colids = np.asarray(colids, dtype=np.int64)
    n = X.shape[0]
    width = (n + PIECE - 1) // PIECE * PIECE
    att = np.zeros(n)
    rep = np.zeros(n)
    for lo in range(0, n, chunk):
        rows = np.arange(lo, min(lo + chunk, n))
        t = X[rows][:, None, :] - X[None, :, :]
        z = pair_sum(t * t, "engine").astype(np.float64)
        terms = np.zeros((len(rows), width))
        terms[:, :n] = -(flog(1e-6 + z) - flog(1.0 + z))
        terms[np.arange(len(rows)), rows] = 0.0
        rep[rows] = _chain(terms, PIECE)
        deg = rowptr[rows + 1] - rowptr[rows]
        dmax = (int(deg.max()) + PIECE - 1) // PIECE * PIECE
        terms = np.zeros((len(rows), max(dmax, PIECE)))
        for r, i in enumerate(rows):
            if deg[r]:
                d = X[i][None, :] - X[colids[rowptr[i]:rowptr[i + 1]]]
                terms[r, :deg[r]] = flog(1.0 + pair_sum(d * d, "engine").astype(np.float64))
        att[rows] = _chain(terms, PIECE)
    pad = np.zeros(width)
    pad[:n] = att
    A = float(_chain(pad[None, :], PIECE)[0])
    pad[:n] = rep
    Rp = float(_chain(pad[None, :], PIECE)[0])
    return A + Rp, A, Rp, int(rowptr[n]), n * (n - 1)
