#!/usr/bin/env python3
"""Time one pass of the GPU logistic regression (include/f2v.h: f2v_logreg_eval -- loss and gradient of every class over all samples)
and whole fits: cora row samples (the node-classification shape: 7 classes), cora pairs (the link-prediction shape: one class,
Hadamard features), and a synthetic m = 1 M, C = 8 case on an RMAT graph.

    python tools/logreg_time.py [--scale 20] [--dim 128] [--reps 5] > profiles/logreg_time.txt

A pass is stated as device seconds (events around its launches: the pass kernel and the reduction of the block sums) and as the bytes
of rows it gathers per second -- m rows of D floats, twice that for pairs -- next to f2v_diag_gather_rate of the same process on a
table the size of the matrix.  A fit's time is the sum over its passes; its wall time adds the host's L-BFGS and one upload of the
weights and one read-back of the sums per pass."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import force2vec_amd as F  # noqa: E402
from force2vec_amd import _lib  # noqa: E402
from force2vec_amd.graph import rmat_csr  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def gather_rate(table_bytes):
    gbps = C.c_double()
    _lib.check(_lib.lib().f2v_diag_gather_rate(0, int(table_bytes), 5, C.byref(gbps)))
    return gbps.value


def time_pass(eng, name, y, reps, ids=None, pairs=None, feature="hadamard"):
    m, classes = y.shape
    W = 0.1 * np.random.default_rng(1).standard_normal((classes, eng.dim + 1))
    eng.logreg_eval(W, y, ids=ids, pairs=pairs, feature=feature)  # warm-up: workspace, code objects
    secs = []
    for _ in range(reps):
        eng.logreg_eval(W, y, ids=ids, pairs=pairs, feature=feature)
        secs.append(eng.last_logreg_seconds)
    t = statistics.median(secs)
    rows = m * (2 if pairs is not None else 1)
    print("%s: m = %d, C = %d: %.3f ms per pass (min %.3f of %d), %.1f GB/s of rows gathered" % (
        name, m, classes, t * 1e3, min(secs) * 1e3, reps, rows * eng.dim * 4 / t * 1e-9), flush=True)


def time_fit(eng, name, y, ids=None, pairs=None):
    t0 = time.perf_counter()
    model = eng.logreg_fit(ids=ids, pairs=pairs, y=y)
    wall = time.perf_counter() - t0
    print("%s: fit of %d classes: %d passes, iterations %s, converged %s: %.3f ms of device time, %.3f ms wall" % (
        name, y.shape[1], int(model.evaluations.max()), model.iterations.tolist(), bool(model.converged.all()), model.seconds * 1e3, wall * 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 20)
    args = ap.parse_args()

    rowptr, colids = F.read_mtx(os.path.join(GOLD, "cora.mtx"))
    n = len(rowptr) - 1
    labels = [[] for _ in range(n)]
    for line in open(os.path.join(GOLD, "cora.nodes.labels")):
        t = line.split()
        if len(t) >= 2:
            labels[int(t[0]) - 1].append(int(t[1]))
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 300, 256, 5, 0.02)
    print("# cora: n = %d, D = %d; 300 epochs of option 5 at batch 256; gather rate on a table of the matrix's size: %.0f GB/s" % (
        n, args.dim, gather_rate(n * args.dim * 4)))
    keep = np.array([v for v in range(n) if labels[v]], dtype=np.uint32)
    classes = len({c for l in labels for c in l})
    y = np.zeros((len(keep), classes), dtype=np.uint8)
    for r, v in enumerate(keep):
        y[r, labels[v]] = 1
    time_pass(eng, "cora rows", y, args.reps, ids=keep)
    cut = len(keep) // 4
    time_fit(eng, "cora rows, a quarter of the labelled vertices", y[:cut], ids=keep[:cut])
    rng = np.random.default_rng(0)
    u = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rowptr).astype(np.int64))
    v = colids.astype(np.uint32)
    neg = rng.integers(0, n, (2 * len(u), 2)).astype(np.uint32)
    pu, pv = np.concatenate([u, neg[:, 0]]), np.concatenate([v, neg[:, 1]])
    py = np.concatenate([np.ones(len(u)), np.zeros(len(neg))]).astype(np.uint8).reshape(-1, 1)
    perm = rng.permutation(len(py))
    pu, pv, py = pu[perm], pv[perm], py[perm]
    time_pass(eng, "cora pairs (hadamard)", py, args.reps, pairs=(pu, pv))
    time_fit(eng, "cora pairs (hadamard)", py, pairs=(pu, pv))
    eng.close()

    rowptr, colids = rmat_csr(args.scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 3, 65536, 5, 0.02)
    epoch = statistics.median(eng.train(5, 1, 65536, 5, 0.02) for _ in range(5))
    print("# RMAT-%d: n = %d, nnz = %d, D = %d; three epochs of option 5 at batch 65536; training epoch %.3f ms; gather rate on a table of the matrix's size: %.0f GB/s" % (
        args.scale, n, eng.nnz, args.dim, epoch * 1e3, gather_rate(n * args.dim * 4)))
    ids = rng.integers(0, n, args.samples).astype(np.uint32)
    for classes in (8, 64):
        y = rng.integers(0, 2, (args.samples, classes)).astype(np.uint8)
        time_pass(eng, "RMAT-%d random rows" % args.scale, y, args.reps, ids=ids)
    y = rng.integers(0, 2, (args.samples, 8)).astype(np.uint8)
    time_pass(eng, "RMAT-%d random pairs (hadamard)" % args.scale, y, args.reps, pairs=(ids, rng.integers(0, n, args.samples).astype(np.uint32)))
    eng.close()


if __name__ == "__main__":
    main()
