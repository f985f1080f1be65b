#!/usr/bin/env python3
"""Time the filtered ranks of held-out edges (include/f2v.h: f2v_pair_ranks) beside the nearest-neighbour query of the same rows.

    python tools/pair_ranks_time.py [--scale 20] [--dim 128] [--frac 0.2] [--edges 65536] [--reps 3] [--nearest-reps 5]
        > profiles/pair_ranks_time.txt

The split of an RMAT graph, then on the training graph's engine (one epoch of option 5: the time is what is measured) `--edges` hidden
edges by the stride rule of Engine.heldout_ranks, both ends, both flags: per metric the device time of the call, of its base-count
launches and of its correction launches ("last_ranks_base_us", "last_ranks_correct_us") and the pairs per second.  The yardstick is
Engine.nearest(k = 10) for the same query rows in the same run: the base pass does the same multiplications and no selection.  The
margin of the comparison is the spread of `--nearest-reps` repetitions of that nearest measurement (after one warm-up)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--frac", type=float, default=0.2)
    ap.add_argument("--edges", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nearest-reps", type=int, default=5)
    ap.add_argument("--metrics", default="dot,l2,cos")
    a = ap.parse_args()
    rowptr, colids = rmat_csr(a.scale)
    n = len(rowptr) - 1
    print("library: %s" % os.environ.get("F2V_LIBRARY", _lib.LIB_PATH), flush=True)
    print("RMAT scale %d: n = %d, nnz = %d; D = %d" % (a.scale, n, len(colids), a.dim), flush=True)
    full = F.Engine(rowptr, colids, 4)
    split = full.edge_split(frac=a.frac, seed=1, ratio=1)
    full.close()
    H = len(split.held_u)
    take = a.edges if 0 < a.edges < H else H
    pick = [j * H // take for j in range(take)]
    u = np.stack([split.held_u[pick], split.held_v[pick]], axis=1).reshape(-1).astype(np.uint32)
    P = len(u)
    print("split frac %g: %d hidden edges, %d of them ranked from both ends: %d pairs; %.3g multiply-adds per call" % (a.frac, H, take, P, float(P) * n * a.dim), flush=True)

    eng = F.Engine(split.rowptr, split.colids, a.dim)
    eng.srand(1)
    eng.init_embeddings(_lib.INIT_SYMMETRIC)
    eng.train(5, 1, 65536)
    pieces = int(sum(-(-(int(split.rowptr[x + 1]) - int(split.rowptr[x])) // 256) for x in u))
    print("correction: %d pair items and %d piece items of 256 nonzeros (the longest row of a ranked u: %d nonzeros)" % (
        P, pieces, max(int(split.rowptr[x + 1]) - int(split.rowptr[x]) for x in u)), flush=True)

    nearest = {}
    for metric in a.metrics.split(","):
        vals = []
        for rep in range(a.nearest_reps + 1):
            eng.nearest(u, k=10, metric=metric, exclude_self=True, exclude_neighbours=True)
            vals.append(eng.last_nearest_seconds)
        vals = vals[1:]
        nearest[metric] = statistics.median(vals)
        print("Engine.nearest(k 10, both flags), %s, %d queries: median %.3f ms on the device, min %.3f max %.3f over %d repetitions (spread %.2f %%) = %.3g queries per second" % (
            metric, P, nearest[metric] * 1e3, min(vals) * 1e3, max(vals) * 1e3, len(vals), 100.0 * (max(vals) - min(vals)) / nearest[metric], P / nearest[metric]), flush=True)
        rows = []
        for rep in range(a.reps + 1):
            t = time.perf_counter()
            r = eng.heldout_ranks(split, metric, sample=take)
            rows.append((r.seconds, eng.get_param("last_ranks_base_us") * 1e-6, eng.get_param("last_ranks_correct_us") * 1e-6, time.perf_counter() - t))
        rows = rows[1:]
        total, base, corr, wall = (statistics.median(x[k] for x in rows) for k in range(4))
        print("f2v_pair_ranks, %s, %d pairs: %.3f ms on the device (base counts %.3f ms, min %.3f max %.3f; correction %.3f ms; targets and gather %.3f ms) = %.3g pairs per second; "
              "%.1f ms wall; base counts / nearest = %.3f (\"ranks_chunk\" %d)" % (
                  metric, P, total * 1e3, base * 1e3, min(x[1] for x in rows) * 1e3, max(x[1] for x in rows) * 1e3, corr * 1e3, (total - base - corr) * 1e3, P / total, wall * 1e3,
                  base / nearest[metric], eng.get_param("ranks_chunk")), flush=True)
        print("    MRR %.6f mean rank %.1f of %d candidates on average; Hits@1 %d Hits@10 %d Hits@50 %d Hits@100 %d of %d; %d tied pairs" % (
            r.mrr, r.mean_rank, r.candidates // max(P, 1), r.hits[1], r.hits[10], r.hits[50], r.hits[100], P, r.tied_pairs), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
