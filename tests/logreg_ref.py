"""TEST INFRASTRUCTURE: numpy restatement of the logistic regression of include/f2v.h (f2v_logreg_eval / _fit / _decision): pair
features in fp32, fp64 fma chains over ascending d for the logits, sums over samples in blocks of 1024 consecutive samples (a block
sequentially from +0, gradient terms by fma, the block sums added in ascending order), the regulariser, and the same L-BFGS.

numpy has no fused multiply-add.  Every fma of the definition has one operand that is an fp32 value (a feature), so its product with
a double is formed exactly as two doubles (the other operand split at 26 bits) and added to the accumulator with one rounding
(`fma24`; checked against exact rational arithmetic by tests/test_logreg.py).

`eval_sums(..., exact=False)` is the same mathematics through BLAS (no fixed order): what the solver tests on the CPU use, where only
the fitted model matters."""
from collections import namedtuple

import numpy as np

BLOCK, MAX_CLASSES = 1024, 64
HADAMARD, L1, L2, AVERAGE = 0, 1, 2, 3
FEATURES = {"hadamard": HADAMARD, "l1": L1, "l2": L2, "average": AVERAGE}

Eval = namedtuple("Eval", "loss grad loss_abs grad_abs z")
Fit = namedtuple("Fit", "weights loss gnorm_inf iterations evaluations converged")


def features(X, a, b=None, feature=HADAMARD):
    """-> float32 [m, D]: rows a, or the pair feature of rows a and b, one fp32 rounding per operation"""
    X = np.asarray(X, dtype=np.float32)
    xa = X[np.asarray(a, dtype=np.int64)]
    if b is None:
        return xa
    xb = X[np.asarray(b, dtype=np.int64)]
    if feature == HADAMARD:
        return xa * xb
    if feature == AVERAGE:
        return (xa + xb) * np.float32(0.5)
    t = xa - xb
    return np.abs(t) if feature == L1 else t * t


def fma24(f, w, acc):
    """round(f * w + acc) with one rounding, elementwise; f holds fp32 values (as float64), w and acc any doubles.  An infinite or NaN
    operand: the plain f * w + acc, which has the fma's value there (the error terms of the two-sum would be inf - inf)."""
    f, w, acc = np.broadcast_arrays(np.asarray(f, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(acc, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        wh = (np.ascontiguousarray(w).view(np.int64) & ~np.int64((1 << 27) - 1)).view(np.float64)
        wl = w - wh                 # exact: at most 27 bits
        ph, pl = f * wh, f * wl     # exact: 24 + 26 and 24 + 27 bits
        s = ph + acc                # two-sum: s + e == ph + acc exactly
        bb = s - ph
        e = (ph - (s - bb)) + (acc - bb)
        return np.where(np.isfinite(s), s + (e + pl), f * w + acc)


def logits(F, W):
    """z [m, C]: the fma chain from +0 over ascending d, then + b; W [C, D + 1], bias last"""
    F = np.asarray(F, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    z = np.zeros((F.shape[0], W.shape[0]))
    for d in range(F.shape[1]):
        z = fma24(F[:, d:d + 1], W[None, :, d], z)
    return z + W[None, :, -1]


def terms(z, y):
    """-> r = sigma(z) - y, l = softplus(z) - y z, as f2v.h writes them"""
    y = np.asarray(y, dtype=np.float64)
    en = np.exp(-np.abs(z))
    sp = np.maximum(z, 0.0) + np.log1p(en)
    sg = np.where(z >= 0.0, 1.0 / (1.0 + en), en / (1.0 + en))
    return sg - y, sp - y * z


def block_sum(a):
    """sum of a 1-D array in the definition's order: blocks of 1024 sequentially from +0, block sums in ascending order"""
    total = 0.0
    for lo in range(0, len(a), BLOCK):
        s = 0.0
        for x in a[lo:lo + BLOCK].tolist():
            s += x
        total += s
    return total


def eval_sums(F, y, W, lam=1.0, exact=True):
    """J and its gradient for every class at W [C, D + 1] -> Eval(loss [C], grad [C, D + 1], and the sums of the absolute values of
    the terms of every entry: what a comparison may lose to cancellation; z [m, C])"""
    F32 = np.asarray(F, dtype=np.float32)
    F = F32.astype(np.float64)
    W = np.asarray(W, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(len(F), -1)
    m, D = F.shape
    C = W.shape[0]
    z = logits(F, W) if exact else F @ W[:, :D].T + W[None, :, D]
    r, l = terms(z, y)
    if exact:
        G, B, S = np.zeros((C, D)), np.zeros(C), np.zeros(C)
        for lo in range(0, m, BLOCK):
            g, b, s = np.zeros((C, D)), np.zeros(C), np.zeros(C)
            for i in range(lo, min(lo + BLOCK, m)):
                g = fma24(F[i][None, :], r[i][:, None], g)
                b = b + r[i]
                s = s + l[i]
            G, B, S = G + g, B + b, S + s
        q = np.zeros(C)
        for d in range(D):
            q = q + W[:, d] * W[:, d]
    else:
        G, B, S = r.T @ F, r.sum(0), l.sum(0)
        q = (W[:, :D] ** 2).sum(1)
    loss = 0.5 * lam * q + S
    grad = np.concatenate([lam * W[:, :D] + G, B[:, None]], axis=1)
    loss_abs = 0.5 * lam * q + np.abs(l).sum(0)
    grad_abs = np.concatenate([np.abs(lam * W[:, :D]) + np.abs(r).T @ np.abs(F), np.abs(r).sum(0)[:, None]], axis=1)
    return Eval(loss, grad, loss_abs, grad_abs, z)


def _direction(g, S, Y, rho):
    q = g.copy()
    alpha = [0.0] * len(S)
    for i in range(len(S) - 1, -1, -1):
        alpha[i] = rho[i] * float(S[i] @ q)
        q -= alpha[i] * Y[i]
    if S:
        q *= float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])
    for i in range(len(S)):
        beta = rho[i] * float(Y[i] @ q)
        q += S[i] * (alpha[i] - beta)
    return -q


def fit(F, y, lam=1.0, tol=1e-4, max_iter=100, exact=False):
    """The solver of f2v.h, every class with its own L-BFGS state, all active classes evaluated in one pass -> Fit"""
    F = np.asarray(F, dtype=np.float32)
    y = np.asarray(y, dtype=np.uint8).reshape(len(F), -1)
    m, D = F.shape
    C = y.shape[1]
    P = D + 1
    stop = tol * m
    ev = eval_sums(F, y, np.zeros((C, P)), lam, exact)
    st = []
    for k in range(C):
        g = ev.grad[k].copy()
        gn = float(np.abs(g).max())
        st.append(dict(w=np.zeros(P), g=g, f=float(ev.loss[k]), S=[], Y=[], rho=[], it=0, ev=1, halvings=0, gn=gn, conv=gn <= stop,
                       active=not gn <= stop and max_iter > 0, searching=False, t=0.0, p=None, gp=0.0, trial=None))
    while True:
        act = [k for k in range(C) if st[k]["active"]]
        if not act:
            break
        for k in act:
            s = st[k]
            if not s["searching"]:
                p = _direction(s["g"], s["S"], s["Y"], s["rho"])
                gp = float(s["g"] @ p)
                if not gp < 0.0:
                    s["S"], s["Y"], s["rho"] = [], [], []
                    p = -s["g"]
                    gp = float(s["g"] @ p)
                s["p"], s["gp"] = p, gp
                s["t"] = 1.0 / float(np.abs(s["g"]).sum()) if s["it"] == 0 else 1.0
                s["halvings"], s["searching"] = 0, True
            s["trial"] = s["w"] + s["t"] * s["p"]
        ev = eval_sums(F, y[:, act], np.stack([st[k]["trial"] for k in act]), lam, exact)
        for i, k in enumerate(act):
            s = st[k]
            s["ev"] += 1
            if ev.loss[i] <= s["f"] + 1e-4 * s["t"] * s["gp"]:
                sv, yv = s["trial"] - s["w"], ev.grad[i] - s["g"]
                sy = float(sv @ yv)
                if sy > 0.0:
                    if len(s["S"]) == 10:
                        s["S"].pop(0), s["Y"].pop(0), s["rho"].pop(0)
                    s["S"].append(sv), s["Y"].append(yv), s["rho"].append(1.0 / sy)
                s["w"], s["g"], s["f"] = s["trial"], ev.grad[i].copy(), float(ev.loss[i])
                s["it"] += 1
                s["searching"] = False
                s["gn"] = float(np.abs(s["g"]).max())
                s["conv"] = s["gn"] <= stop
                if s["conv"] or s["it"] >= max_iter:
                    s["active"] = False
            else:
                s["halvings"] += 1
                if s["halvings"] > 40:
                    s["active"] = False
                else:
                    s["t"] *= 0.5
    col = lambda name, dtype: np.array([s[name] for s in st], dtype=dtype)
    return Fit(np.stack([s["w"] for s in st]), col("f", np.float64), col("gn", np.float64), col("it", np.uint32), col("ev", np.uint32),
               col("conv", bool))


def f1(true, pred, classes):
    """micro / macro F1 in percent of 0/1 matrices over the class columns `classes` (an empty class scores 0)"""
    t, p = np.asarray(true)[:, classes].astype(bool), np.asarray(pred)[:, classes].astype(bool)
    tp, fp, fn = (t & p).sum(0).astype(np.float64), (~t & p).sum(0).astype(np.float64), (t & ~p).sum(0).astype(np.float64)
    den = 2 * tp + fp + fn
    per = np.where(den > 0, 2 * tp / np.where(den > 0, den, 1), 0.0)
    return 100.0 * 2 * tp.sum() / max(den.sum(), 1.0), 100.0 * float(per.mean())


def top_k(z, true):
    """every row predicted as many labels as it truly has: the largest z, ties to the lower class"""
    order = np.argsort(-z, axis=1, kind="stable")
    pred = np.zeros_like(true)
    for r in range(len(true)):
        pred[r, order[r, :int(true[r].sum())]] = 1
    return pred


def onehot(labels, ids, classes):
    y = np.zeros((len(ids), classes), dtype=np.uint8)
    for r, v in enumerate(ids):
        y[r, labels[v]] = 1
    return y


def classify(X, labels, train_ids, test_ids, classes, **kw):
    """-> (micro, macro) F1 in percent of the restated solver on rows of X"""
    X = np.asarray(X, dtype=np.float32)
    model = fit(X[train_ids], onehot(labels, train_ids, classes), **kw)
    Ft = X[test_ids].astype(np.float64)
    z = Ft @ model.weights[:, :-1].T + model.weights[None, :, -1]
    true = onehot(labels, test_ids, classes)
    return f1(true, top_k(z, true), np.arange(classes))


def link_predict(X, pairs, train_frac=0.5, feature=HADAMARD, **kw):
    """-> (accuracy, F1-macro, F1-micro) in percent, as runlinkpredict.py:127-140 scores it"""
    u, v, y = (np.asarray(a) for a in pairs)
    F = features(X, u, v, feature)
    cv = int(len(y) * train_frac)
    model = fit(F[:cv], y[:cv].reshape(-1, 1), **kw)
    z = F[cv:].astype(np.float64) @ model.weights[0, :-1] + model.weights[0, -1]
    pred, true = (z > 0).astype(np.uint8), y[cv:].astype(np.uint8)
    two = lambda a: np.stack([a == 0, a == 1], axis=1)
    micro, macro = f1(two(true), two(pred), np.unique(pred))
    return 100.0 * float((pred == true).mean()), macro, micro
