"""numpy restatement of the t-SNE definition of include/f2v.h (tests/test_tsne.py, tools/): the neighbours (the order of
tests/nearest_ref.py among the laid-out points alone), scikit-learn's binary search for the conditional affinities, the symmetric
sparse P, and the iteration -- pair arithmetic in fp32, repulsion in pieces of 64 columns and spans of 16 pieces, attraction and the
Kullback-Leibler sum in pieces of 64 entries, Z and KL over pieces of 64 rows, the gradient-descent step in fp64.

Two modes.  exact=True walks every sum in the definition's order (vectorised ACROSS rows and pieces, sequential INSIDE them) and is
bit for bit what the kernels return when both sides start from the same P: exp and log of the binary search are the one place where
host and device agree to a tolerance.  exact=False uses numpy's own sums, for long runs whose quality is what is asked.
Nothing here knows how the kernels tile, stage or place their work."""
from collections import namedtuple

import numpy as np

import exact_ref as E
import nearest_ref as R

PIECE, SPAN = 64, 16
TINY = np.finfo(np.float64).tiny
F32, F64 = np.float32, np.float64
Result = namedtuple("Result", "y kl z learning_rate kl_iters kl_values")


def neighbours(X, k):
    """(ids [m, k], d [m, k] float64): the k nearest of every row among the rows of X, itself excluded, and their squared distances."""
    X = np.ascontiguousarray(X, dtype=F32)
    ids, scores = R.nearest_ref(X, k, "l2", qids=np.arange(len(X)), exclude_self=True)
    return ids, (-scores).astype(F64)


def conditionals(d, perplexity):
    """scikit-learn's _binary_search_perplexity in fp64 on the k distances of every point -> (p_(j|i) [m, k], entropies [m])."""
    d = np.asarray(d, dtype=F64)
    m, k = d.shape
    beta, lo, hi = np.ones(m), np.full(m, -np.inf), np.full(m, np.inf)
    target = np.log(perplexity)
    P, H = np.zeros((m, k)), np.zeros(m)
    active = np.ones(m, dtype=bool)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for step in range(100):
            at = np.nonzero(active)[0]
            if not len(at):
                break
            b, da = beta[at], d[at]
            p = np.exp(-b[:, None] * da)
            S, T = np.zeros(len(at)), np.zeros(len(at))
            for j in range(k):
                S = S + p[:, j]
                T = T + da[:, j] * p[:, j]
            S = np.where(S == 0.0, 1e-8, S)
            H[at] = np.log(S) + (b * T) / S
            P[at] = p / S[:, None]
            diff = H[at] - target
            done = np.abs(diff) <= 1e-5
            if step == 99:
                break
            up = diff > 0.0
            lo[at] = np.where(up & ~done, b, lo[at])
            hi[at] = np.where(~up & ~done, b, hi[at])
            nb = np.where(up, np.where(np.isinf(hi[at]), b * 2.0, (b + hi[at]) / 2.0), np.where(np.isinf(lo[at]), b / 2.0, (b + lo[at]) / 2.0))
            beta[at] = np.where(done, b, nb)
            active[at[done]] = False
    return P, H


def symmetric(ids, cond):
    """(rowptr uint32 [m + 1], colids uint32, values float64) of p_ij = (p_(j|i) + p_(i|j)) / (2.0 m), entries below the smallest
    normal double dropped, column ids ascending inside a row."""
    m = len(ids)
    C = np.zeros((m, m))
    has = np.zeros((m, m), dtype=bool)
    rows = np.repeat(np.arange(m), ids.shape[1])
    C[rows, ids.reshape(-1)] = cond.reshape(-1)
    has[rows, ids.reshape(-1)] = True
    P = (C + C.T) / (2.0 * m)
    keep = (has | has.T) & ~(P < TINY)
    r, c = np.nonzero(keep)  # row-major: ascending columns inside a row
    rowptr = np.zeros(m + 1, dtype=np.uint32)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=m))
    return rowptr, c.astype(np.uint32), P[r, c]


def affinities(X, perplexity):
    ids, d = neighbours(X, int(np.floor(3.0 * perplexity)))
    return symmetric(ids, conditionals(d, perplexity)[0])


def _seq(terms):
    """[..., q] -> the sequential sum from +0 over the last axis."""
    acc = np.zeros(terms.shape[:-1], dtype=terms.dtype)
    for q in range(terms.shape[-1]):
        acc = acc + terms[..., q]
    return acc


def _pad(a, multiple, axis):
    extra = -a.shape[axis] % multiple
    if not extra:
        return a
    width = [(0, 0)] * a.ndim
    width[axis] = (0, extra)
    return np.pad(a, width)  # zeros: adding +0 to a sum that began at +0 changes no bit


def _pieces(terms, width):
    """[rows, L, ...] -> per row: pieces of `width` along axis 1, each summed sequentially from +0, the piece sums added sequentially."""
    t = np.moveaxis(_pad(terms, width, 1), 1, -1)
    t = t.reshape(t.shape[:-1] + (-1, width))
    return _seq(_seq(t))


def _pair(yi, yj):
    """t, w of pair(i, j) on float32 arrays [..., d2]: every operation one rounded fp32 operation."""
    t = yi - yj
    a = t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]
    if t.shape[-1] == 3:
        a = a + t[..., 2] * t[..., 2]
    return t, F32(1) / (F32(1) + a)


class _Csr:
    def __init__(self, rowptr, colids, values, m):
        rowptr = np.asarray(rowptr, dtype=np.int64)
        length = np.diff(rowptr)
        L = max(int(length.max()), 1)
        self.valid = np.arange(L)[None, :] < length[:, None]
        at = np.minimum(rowptr[:-1, None] + np.arange(L)[None, :], max(len(colids) - 1, 0))
        self.cols = np.where(self.valid, np.asarray(colids, dtype=np.int64)[at], 0)
        self.vals = np.where(self.valid, np.asarray(values, dtype=F64)[at], 1.0)


def _repulsion(yf, exact):
    """Z_i [m], R_i [m, d2], Z"""
    m, d2 = yf.shape
    if not exact:  # the same pair arithmetic, numpy's own sums
        t = [yf[:, None, d] - yf[None, :, d] for d in range(d2)]
        a = t[0] * t[0] + t[1] * t[1]
        if d2 == 3:
            a = a + t[2] * t[2]
        w = F32(1) / (F32(1) + a)
        np.fill_diagonal(w, F32(0))
        Zi, ww = w.sum(1, dtype=F64), w * w
        return Zi, np.stack([(ww * td).sum(1, dtype=F64) for td in t], axis=1), float(Zi.sum())
    t, w = _pair(yf[:, None, :], yf[None, :, :])
    w = np.where(np.eye(m, dtype=bool), F32(0), w)  # j == i is left out
    r = (w * w)[:, :, None] * t
    zp = _seq(_pad(w, PIECE, 1).reshape(m, -1, PIECE)).astype(F64)  # fp32 piece sums, converted
    rp = _seq(np.moveaxis(_pad(r, PIECE, 1), 1, -1).reshape(m, d2, -1, PIECE)).astype(F64)
    Zi = _seq(_seq(_pad(zp, SPAN, 1).reshape(m, -1, SPAN)))
    Ri = _seq(_seq(_pad(rp, SPAN, 2).reshape(m, d2, -1, SPAN)))
    return Zi, Ri, float(_seq(_seq(_pad(Zi, PIECE, 0).reshape(-1, PIECE))))


def _attraction(yf, csr, ex, exact):
    t, w = _pair(yf[:, None, :], yf[csr.cols])
    term = np.where(csr.valid[:, :, None], ((ex * csr.vals) * w.astype(F64))[:, :, None] * t.astype(F64), 0.0)
    return _pieces(term, PIECE) if exact else term.sum(1)


def kl_divergence(yf, csr, Z, exact=True):
    _, w = _pair(yf[:, None, :], yf[csr.cols])
    term = np.where(csr.valid, csr.vals * (E.flog(csr.vals) - (E.flog(w.astype(F64)) - E.flog(np.array([Z]))[0])), 0.0)
    rows = _pieces(term, PIECE) if exact else term.sum(1)
    return float(_seq(_seq(_pad(rows, PIECE, 0).reshape(-1, PIECE)))) if exact else float(rows.sum())


def pca_start(proj, variance0):
    """scikit-learn's init = "pca" scaling of an fp32 projection (f2v_pca's, the rows of the sample)."""
    return np.asarray(proj, dtype=F32).astype(F64) * (1e-4 / np.sqrt(F64(variance0)))


def run(P, y0, iters=1000, exaggeration=12.0, exaggeration_iters=250, learning_rate=None, kl_every=0, exact=True):
    """The iteration of the definition from P = (rowptr, colids, values) and the start y0 [m, d2] float64 -> Result."""
    y = np.array(y0, dtype=F64)
    m, d2 = y.shape
    csr = _Csr(P[0], P[1], P[2], m)
    lr = float(learning_rate) if learning_rate else max(float(m) / exaggeration / 4.0, 50.0)
    update, gains = np.zeros_like(y), np.ones_like(y)
    kl_iters, kl_values = [], []
    kl = z = float("nan")
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for it in range(iters):
            early = it < exaggeration_iters
            yf = y.astype(F32)
            _, Ri, Z = _repulsion(yf, exact)
            A = _attraction(yf, csr, exaggeration if early else 1.0, exact)
            g = 4.0 * (A - Ri / Z)
            gains = np.where(update * g < 0.0, gains + 0.2, gains * 0.8)
            gains = np.where(gains < 0.01, 0.01, gains)
            g = g * gains
            update = (0.5 if early else 0.8) * update - lr * g
            y = y + update
            last, log = it + 1 == iters, bool(kl_every) and (it + 1) % kl_every == 0
            if last or log:
                yf = y.astype(F32)
                z = _repulsion(yf, exact)[2]
                kl = kl_divergence(yf, csr, z, exact)
                if log:
                    kl_iters.append(it + 1)
                    kl_values.append(kl)
    return Result(y.astype(F32), kl, z, lr, np.array(kl_iters, dtype=np.uint32), np.array(kl_values, dtype=F64))


def blobs(seed=5, centres=8, per=75, D=32, spread=0.45):
    """The test data: `centres` centres N(0, 1) in D dimensions, `per` points each at spread x N(0, 1), float32.  (With seed 5 a PCA
    layout has a trustworthiness of 0.887 at k = 5: blobs that a linear projection lays over each other.)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, D))
    return (np.repeat(c, per, axis=0) + spread * rng.standard_normal((centres * per, D))).astype(F32)
