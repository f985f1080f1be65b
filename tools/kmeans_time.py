#!/usr/bin/env python3
"""Time the GPU k-means (include/f2v.h: clustering) on an RMAT graph: device time per Lloyd iteration at K = 8 / 64 / 1024 from
info.seconds over runs of `--iters` iterations (noise rarely converges that early; the iterations actually run are divided by), a full
restarts = 10 clustering at K = 25, one f2v_modularity call, and beside them the training epoch at batch 65536 and the
f2v_diag_stream_copy rate of the same process.

    python tools/kmeans_time.py [--scale 20] [--dim 128] [--iters 20] > profiles/kmeans_time.txt
    rocprofv3 --kernel-trace --stats -d /tmp/km_prof -- python tools/kmeans_time.py --profile-pass     # the kernel split

Each per-iteration figure is stated against its floor: for K = 8 and 64 two reads of the matrix (assignment and piece sums:
2 N D 4 bytes) at the measured copy rate -- the copy rate counts read + written bytes, so that is the rate bytes cross HBM at -- and
for K = 1024 the 3 N K D vector operations (subtract, and the fma counted as two) at the 157.3 TF fp32 vector peak.
info.seconds lies between two events around the call's launches, so a per-iteration figure carries the iteration's launch gaps and
its blocking 4-byte read-back of the changed-label count (the seeded rows are chosen before the first event); the kernels' own
time is what the --profile-pass shows."""
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

PEAK_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-pass", action="store_true", help="one warm run per K and nothing else (run under rocprofv3)")
    args = ap.parse_args()
    rowptr, colids = rmat_csr(args.scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 3, 65536, 5, 0.02)
    print("# RMAT-%d: n = %d, nnz = %d, D = %d; three epochs of option 5 at batch 65536" % (args.scale, n, eng.nnz, args.dim))
    if args.profile_pass:
        for k in (8, 64, 1024):
            eng.kmeans(k, 2, seed=1)
            res = eng.kmeans(k, args.iters, seed=1)
            print("K=%d: %d iterations, %.6f s" % (k, res.iterations, eng.last_kmeans_seconds))
        eng.modularity(res.labels, 1024)
        return
    gbps = C.c_double()
    _lib.check(_lib.lib().f2v_diag_stream_copy(0, 1 << 30, 5, C.byref(gbps)))
    epoch = statistics.median(eng.train(5, 1, 65536, 5, 0.02) for _ in range(5))
    print("stream copy (read + written bytes): %.0f GB/s; training epoch at batch 65536: %.3f ms" % (gbps.value, epoch * 1e3))
    mem_floor = 2.0 * n * args.dim * 4 / (gbps.value * 1e9)
    print("# per-iteration figures: event time of the whole call / iterations -- kernels, launch gaps and one blocking 4-byte read-back per iteration")
    for k in (8, 64, 1024):
        eng.kmeans(k, 2, seed=1)  # warm-up: workspace, code objects
        per = []
        for _ in range(args.reps):
            res = eng.kmeans(k, args.iters, seed=1)
            per.append(eng.last_kmeans_seconds / max(res.iterations, 1))
        t = statistics.median(per)
        alu_floor = 3.0 * n * k * args.dim / (PEAK_TF * 1e12)
        which = "memory" if mem_floor >= alu_floor else "vector ALU"
        floor = max(mem_floor, alu_floor)
        print("K=%-4d %.3f ms per Lloyd iteration (min %.3f, %d runs of %d iterations) | floors: memory %.3f ms, vector ALU %.3f ms -> %s bound applies: %.2f x its floor | %.2f training epochs"
              % (k, t * 1e3, min(per) * 1e3, args.reps, res.iterations, mem_floor * 1e3, alu_floor * 1e3, which, t / floor, t / epoch), flush=True)
    for k in (8, 1024):  # rows per workgroup of the assignment kernel ("kmeans_block"; 0 picks 64 at these K)
        for block in (64, 128, 256):
            eng.set_param("kmeans_block", block)
            eng.kmeans(k, 1, seed=1)
            res = eng.kmeans(k, 5, seed=1)
            print("K=%-4d kmeans_block=%-3d %.3f ms per Lloyd iteration (one run of %d)" % (k, block, eng.last_kmeans_seconds / max(res.iterations, 1) * 1e3, res.iterations), flush=True)
    eng.set_param("kmeans_block", 0)
    t0 = time.perf_counter()
    res = eng.kmeans(25, 300, seed=1, restarts=10)
    wall = time.perf_counter() - t0
    print("K=25 restarts=10 max_iters=300: %.3f s of device time, %.3f s wall; restart %d won after %d iterations (converged %s), inertia %.9g"
          % (eng.last_kmeans_seconds, wall, res.restart, res.iterations, res.converged, res.inertia), flush=True)
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        m = eng.modularity(res.labels, 25)
        walls.append(time.perf_counter() - t0)
    print("f2v_modularity(25 clusters): Q = %.6f over %d edges, %.3f ms wall per call (labels uploaded, tallies read back)" % (m.q, m.edges, min(walls) * 1e3))
    eng.close()


if __name__ == "__main__":
    main()
