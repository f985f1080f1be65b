#!/usr/bin/env python3
"""Time the GPU separation scores (include/f2v.h: separation) on an RMAT graph: f2v_silhouette for 8192, 65536 and all samples and
f2v_davies_bouldin, on the matrix after three epochs of option 5 with the labels of a kmeans(64) run; medians of `--reps` calls of
the device time the calls report (events around their own launches).

    python tools/separation_time.py [--scale 20] [--dim 128] [--clusters 64] > profiles/separation_time.txt
    python tools/separation_time.py --samples 8192 65536          # leave the all-samples call out (it takes seconds)
    rocprofv3 --kernel-trace --stats -d /tmp/sep_prof -- python tools/separation_time.py --profile-pass     # the kernel split

Each figure is stated against its floor.  The silhouette's is the vector ALU's: a pair and dimension costs a subtraction and an fma,
2 vector operations, over the UNPACKED fp32 issue rate (78.6 T operations/s: half the 157.3 TF peak, which counts an fma as two and
assumes packed instructions) -- and half that time where both are packed (separation_pair_kernel packs a lane's two sample rows).
The Davies-Bouldin score's is the memory's: two reads of the matrix (the centroids' piece sums, the scatter) at the measured copy
rate, which counts read + written bytes and so is the rate bytes cross HBM at."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import force2vec_amd as F  # noqa: E402
from force2vec_amd import _lib  # noqa: E402
from force2vec_amd.graph import rmat_csr  # noqa: E402

UNPACKED_TOPS = 157.3 / 2  # fp32 vector instructions issued per second, in units of 1e12 lanes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--clusters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="*", default=[8192, 65536, 0], help="sample counts (0 = every vertex)")
    ap.add_argument("--blocks", type=int, nargs="*", default=[64, 128], help="\"separation_block\" values tried at the first sample count")
    ap.add_argument("--profile-pass", action="store_true", help="one call per sample count below 100000 and nothing else (run under rocprofv3)")
    args = ap.parse_args()
    rowptr, colids = rmat_csr(args.scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 3, 65536, 5, 0.02)
    labels = eng.kmeans(args.clusters, 20, seed=1).labels
    counts = np.bincount(labels, minlength=args.clusters)
    print("# RMAT-%d: n = %d, nnz = %d, D = %d; three epochs of option 5 at batch 65536; labels of kmeans(%d, 20 iterations): clusters of %d .. %d members, %d spans"
          % (args.scale, n, eng.nnz, args.dim, args.clusters, counts.min(), counts.max(), int(((counts + 4095) // 4096).sum())), flush=True)
    order = np.random.default_rng(1).permutation(n).astype(np.uint32)
    if args.profile_pass:
        for m in args.samples:
            if 0 < m < 100000:
                eng.silhouette(labels, order[:m])
                print("samples=%d: %.6f s" % (m, eng.last_separation_seconds))
        eng.davies_bouldin(labels)
        return
    gbps = C.c_double()
    _lib.check(_lib.lib().f2v_diag_stream_copy(0, 1 << 30, 5, C.byref(gbps)))
    print("stream copy (read + written bytes): %.0f GB/s" % gbps.value)
    eng.silhouette(labels, order[:256])  # warm-up: workspace, code objects
    for m in args.samples:
        ids = None if m == 0 else order[:m]
        nq = n if m == 0 else m
        times = []
        for _ in range(args.reps if m else 1):
            score = eng.silhouette(labels, ids)
            times.append(eng.last_separation_seconds)
        t = statistics.median(times)
        floor = 2.0 * nq * n * args.dim / (UNPACKED_TOPS * 1e12)
        print("f2v_silhouette samples=%-8d %.3f ms (min %.3f, %d calls) = %.4f | vector-ALU floor %.3f ms unpacked (%.2f x), %.3f ms packed (%.2f x) | %.2f T pair-dimensions/s"
              % (nq, t * 1e3, min(times) * 1e3, len(times), score, floor * 1e3, t / floor, floor * 0.5e3, 2 * t / floor, nq * n * args.dim / t * 1e-12), flush=True)
    m = [s for s in args.samples if s][:1]
    for block in args.blocks if m else []:
        eng.set_param("separation_block", block)
        eng.silhouette(labels, order[:m[0]])
        times = []
        for _ in range(args.reps):
            eng.silhouette(labels, order[:m[0]])
            times.append(eng.last_separation_seconds)
        print("f2v_silhouette samples=%-8d separation_block=%-3d %.3f ms" % (m[0], block, statistics.median(times) * 1e3), flush=True)
    eng.set_param("separation_block", 0)
    eng.davies_bouldin(labels)
    times = []
    for _ in range(args.reps):
        score = eng.davies_bouldin(labels)
        times.append(eng.last_separation_seconds)
    t = statistics.median(times)
    floor = 2.0 * n * args.dim * 4 / (gbps.value * 1e9)
    print("f2v_davies_bouldin %.3f ms (min %.3f, %d calls) = %.4f | memory floor (two reads of the matrix) %.3f ms: %.2f x its floor" % (
        t * 1e3, min(times) * 1e3, len(times), score, floor * 1e3, t / floor), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
