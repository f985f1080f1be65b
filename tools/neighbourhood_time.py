#!/usr/bin/env python3
"""Time the neighbourhood scores of pairs (include/f2v.h: f2v_pair_neighbourhood) on the held-out set of an RMAT graph.

    python tools/neighbourhood_time.py [--scale 20] [--frac 0.2] [--ratio 1] [--reps 3] [--host-pairs 1048576]
        > profiles/neighbourhood_time.txt

The split of tools/heldout_time.py (RMAT, frac, ratio, seed 1), then on the training graph's engine, for the hidden edges and the
negatives: the device time of all five kinds, of common neighbours alone and of the degree product alone; the share of pairs whose S
row has more than one piece of 1024 nonzeros; the single most expensive pair alone; the whole set with the pieces as work items of
their own ("neighbourhood_spread" 1, the default) and with one wavefront per pair (0); and, for context, the host time of scipy.sparse
counting the common neighbours of the first --host-pairs pairs (checked against the engine's counts)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import force2vec_amd as F  # noqa: E402
from force2vec_amd import _lib  # noqa: E402
from force2vec_amd.graph import rmat_csr  # noqa: E402


def timed(eng, u, v, kinds, reps):
    """-> (median device seconds over `reps` calls after one warm-up, median wall seconds, the last result)"""
    dev, wall, out = [], [], None
    for _ in range(reps + 1):
        t = time.perf_counter()
        out = eng.pair_neighbourhood(u, v, kinds)
        wall.append(time.perf_counter() - t)
        dev.append(eng.last_neighbourhood_seconds)
    return statistics.median(dev[1:]), statistics.median(wall[1:]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--frac", type=float, default=0.2)
    ap.add_argument("--ratio", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=1 << 20)
    a = ap.parse_args()
    rowptr, colids = rmat_csr(a.scale)
    n = len(rowptr) - 1
    print("library: %s" % os.environ.get("F2V_LIBRARY", os.path.relpath(_lib.LIB_PATH, ROOT)), flush=True)
    print("RMAT scale %d: n = %d, nnz = %d" % (a.scale, n, len(colids)), flush=True)
    full = F.Engine(rowptr, colids, 4)
    split = full.edge_split(frac=a.frac, seed=1, ratio=a.ratio)
    full.close()
    u, v = np.concatenate([split.held_u, split.neg_u]), np.concatenate([split.held_v, split.neg_v])
    m = len(u)
    length = np.diff(split.rowptr.astype(np.int64))
    print("training graph (frac %g, ratio %d): nnz = %d, longest row %d; %d hidden edges + %d negatives = %d pairs" % (
        a.frac, a.ratio, len(split.colids), length.max(), len(split.held_u), len(split.neg_u), m), flush=True)
    short, long_ = np.minimum(length[u], length[v]), np.maximum(length[u], length[v])
    pieces = -(-short // 1024)
    several = pieces > 1
    print("pairs whose S row has more than one piece: %d of %d (share %.3g), %d pieces in all, the most %d; nonzeros of S rows in all %d, %.3g of them in those pairs" % (
        several.sum(), m, several.mean(), pieces[several].sum(), pieces.max(), short.sum(), short[several].sum() / max(short.sum(), 1)), flush=True)

    eng = F.Engine(split.rowptr, split.colids, 4)
    chunk = eng.get_param("pairs_chunk")
    for name, kinds in (("all five kinds", ("cn", "jaccard", "aa", "ra", "pa")), ("common neighbours alone", ("cn",)), ("the degree product alone", ("pa",))):
        dev, wall, out = timed(eng, u, v, kinds, a.reps)
        print("f2v_pair_neighbourhood, %s (%d pairs): %.3f ms on the device = %.3g pairs per second; %.1f ms wall (\"pairs_chunk\" %d, %d piece items)" % (
            name, m, dev * 1e3, m / dev, wall * 1e3, chunk, eng.get_param("last_neighbourhood_items")), flush=True)
        if "cn" in kinds:
            cn = out["cn"]
    worst = int(np.argmax(short * np.log2(long_ + 2.0)))  # searches times steps: the pair with the most work
    one_u, one_v = u[worst:worst + 1], v[worst:worst + 1]
    for spread in (1, 0):
        eng.set_param("neighbourhood_spread", spread)
        dev_all, _, _ = timed(eng, u, v, ("cn", "jaccard", "aa", "ra", "pa"), a.reps)
        dev_one, _, _ = timed(eng, one_u, one_v, ("cn", "jaccard", "aa", "ra", "pa"), a.reps)
        print("\"neighbourhood_spread\" %d: all five kinds of the whole set %.3f ms on the device; the most expensive pair alone (%d, %d): S row %d nonzeros = %d pieces, "
              "L row %d: %.3f ms" % (spread, dev_all * 1e3, one_u[0], one_v[0], short[worst], pieces[worst], long_[worst], dev_one * 1e3), flush=True)
    eng.close()

    from scipy.sparse import csr_matrix
    k = min(a.host_pairs, m)
    t = time.perf_counter()
    A = csr_matrix((np.ones(len(split.colids), dtype=np.int32), split.colids.astype(np.int64), split.rowptr.astype(np.int64)), shape=(n, n))
    A.sum_duplicates()
    A.setdiag(0)
    A.eliminate_zeros()
    A.data[:] = 1
    built = time.perf_counter() - t
    t = time.perf_counter()
    host = np.empty(k, dtype=np.int64)
    for lo in range(0, k, 1 << 16):
        hi = min(lo + (1 << 16), k)
        host[lo:hi] = np.asarray(A[u[lo:hi]].multiply(A[v[lo:hi]]).sum(axis=1)).reshape(-1)
    took = time.perf_counter() - t
    same = bool(np.array_equal(host.astype(np.float64), cn[:k]))
    print("scipy.sparse on the host, common neighbours of the first %d pairs (row slices multiplied, 65536 pairs a block): %.1f ms + %.1f ms for the matrix "
          "= %.3g pairs per second; equal to the engine's counts: %s" % (k, took * 1e3, built * 1e3, k / took, same), flush=True)


if __name__ == "__main__":
    main()
