#!/usr/bin/env python3
"""Time the inverted-file index (include/f2v.h, "nearest neighbours through an index") against the exact search of the same build on an
RMAT graph: the build at `--lists` lists split into k-means and sort, then for nq = 1 / 1024 / 65536 and nprobe = 1 / 4 / 16 / 64 the
device seconds of index_search for dot, L2 and cosine, its recall@k against nearest() on the same queries, and nearest()'s own time in
the same process, interleaved with the index's calls rep by rep (as profiles/nearest_time.txt was made).  One GPU step: run it under
a time limit of its own,

    timeout -k 10 900 python tools/index_time.py [--scale 20] [--dim 128] [--k 10] > profiles/index_time.txt
    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/index_time.py --profile-pass     # the kernel split

Reported per case: median and minimum time, the speed-up over the exact search, candidates per query, the efficiency
exact_time x (candidates / (nq n)) / index_time -- how close the scan comes to "time in proportion to the rows scored" -- and the
recall; at the end, per metric and nq, the smallest measured nprobe with recall >= 0.9."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import force2vec_amd as F  # noqa: E402
from force2vec_amd.graph import rmat_csr  # noqa: E402

PAD = 0xFFFFFFFF


def recall(got, want):
    found = ((got[:, None, :] == want[:, :, None]).any(axis=2) & (want != PAD)).sum()
    return float(found) / max(1, int((want != PAD).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--profile-pass", action="store_true", help="two warm searches per metric at nq = 65536, nprobe = 16 and nothing else (run under rocprofv3)")
    args = ap.parse_args()
    rowptr, colids = rmat_csr(args.scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, args.epochs, 65536, 5, 0.02)
    print("# RMAT-%d: n = %d, nnz = %d, D = %d, k = %d; %d epochs of option 5" % (args.scale, n, eng.nnz, args.dim, args.k, args.epochs))
    eng.kmeans(args.lists, max_iters=1, seed=1)  # warm-up (workspace, code objects)
    km = eng.kmeans(args.lists, max_iters=args.iters, seed=1)
    t_km = eng.last_kmeans_seconds
    eng.build_index(labels=km.labels, centroids=km.centroids)
    t_sort = statistics.median(eng.build_index(labels=km.labels, centroids=km.centroids).seconds for _ in range(5))
    info = eng.build_index(lists=args.lists, max_iters=args.iters, seed=1)
    print("build: lists = %d, k-means %.6f s (%d iterations, converged %d) + sort into list order %.6f s; f2v_index_build as one call %.6f s; "
          "largest list %d, empty lists %d, %.1f MB" % (info.lists, t_km, km.iterations, km.converged, t_sort, info.seconds, info.largest, info.empty, info.bytes / 1e6),
          flush=True)
    rng = np.random.default_rng(1)
    if args.profile_pass:
        q = rng.choice(n, 65536, replace=False).astype(np.uint32)
        for metric in ("dot", "l2", "cos"):
            for _ in range(2):
                eng.index_search(ids=q, k=args.k, metric=metric, nprobe=16)
            print("%s nq=65536 nprobe=16: %.6f s" % (metric, eng.last_nearest_seconds))
        return
    probes = (1, 4, 16, 64)
    print("# case: index median s (min s over reps) | exact median s | speed-up | candidates/query | efficiency | recall@%d" % args.k)
    enough = {}
    for nq, reps in ((1, 10), (1024, 10), (65536, 3)):
        q = rng.choice(n, nq, replace=False).astype(np.uint32)
        for metric in ("dot", "l2", "cos"):
            want, _ = eng.nearest(ids=q, k=args.k, metric=metric)  # warm-up of both paths, and the recall's yardstick
            got, cand = {}, {}
            for p in probes:
                ids, _, _, d = eng.index_search(ids=q, k=args.k, metric=metric, nprobe=p, details=True)
                got[p], cand[p] = ids, d["candidates"]
            exact, ours = [], {p: [] for p in probes}
            for _ in range(reps):  # interleaved: both see the same clocks
                eng.nearest(ids=q, k=args.k, metric=metric)
                exact.append(eng.last_nearest_seconds)
                for p in probes:
                    eng.index_search(ids=q, k=args.k, metric=metric, nprobe=p)
                    ours[p].append(eng.last_nearest_seconds)
            te = statistics.median(exact)
            for p in probes:
                t, r = statistics.median(ours[p]), recall(got[p], want)
                if r >= 0.9:
                    enough.setdefault((metric, nq), p)
                print("%-4s nq=%-6d nprobe=%-3d %.6f s (min %.6f, %d reps) | exact %.6f s | %7.2f x | %10.1f | %.3f | %.4f"
                      % (metric, nq, p, t, min(ours[p]), reps, te, te / t, cand[p] / nq, te * (cand[p] / (nq * n)) / t, r), flush=True)
    for (metric, nq), p in sorted(enough.items()):
        print("smallest measured nprobe with recall@%d >= 0.9: %-4s nq=%-6d %d" % (args.k, metric, nq, p))
    eng.close()


if __name__ == "__main__":
    main()
