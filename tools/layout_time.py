#!/usr/bin/env python3
"""Time the GPU layout calls (include/f2v.h: layout): f2v_pca(2) on an RMAT graph against one streaming read of the matrix, the
rank kernel of f2v_trustworthiness against f2v_silhouette on the same n, D and samples (the same distances, another epilogue), and
whole f2v_trustworthiness calls for the PCA layout of a trained cora embedding and of the RMAT matrix with a 4096-vertex sample;
medians of `--reps` calls of the device time the calls report (events around their own launches).

    python tools/layout_time.py [--scale 20] [--small-scale 16] [--dim 128] > profiles/layout_time.txt

The rank kernel's rate is taken from a call with Y = X (both directions then rank in D dimensions) less two nearest-neighbour
queries of the same samples, which the call also holds."""
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


def median(call, reps):
    call()
    times = [call() for _ in range(reps)]
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--small-scale", type=int, default=16)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cora", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cora.mtx"))
    args = ap.parse_args()
    gbps = C.c_double()
    _lib.check(_lib.lib().f2v_diag_stream_copy(0, 1 << 30, 5, C.byref(gbps)))
    print("stream copy (read + written bytes): %.0f GB/s" % gbps.value, flush=True)

    # 2. the rank kernel against the silhouette's pair kernel
    rowptr, colids = rmat_csr(args.small_scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 3, 65536, 5, 0.02)
    X = eng.get_embeddings()
    ids = np.random.default_rng(1).permutation(n)[:8192].astype(np.uint32)
    labels = eng.kmeans(64, 20, seed=1).labels

    def sil():
        eng.silhouette(labels, ids)
        return eng.last_separation_seconds

    def nn():
        eng.nearest(ids=ids, k=5, metric="l2")
        return eng.last_nearest_seconds

    t_sil, t_nn = median(sil, args.reps)[0], median(nn, args.reps)[0]
    for block in (0, 128):
        eng.set_param("trust_block", block)
        t_xx = median(lambda: eng.trustworthiness(X, 5, ids).seconds, args.reps)[0]
        rank = (t_xx - 2 * t_nn) / 2
        pd = len(ids) * n * args.dim
        print("RMAT-%d n=%d D=%d, 8192 samples, k=5, trust_block=%d: f2v_trustworthiness(Y = X) %.3f ms, f2v_nearest_rows %.3f ms -> one rank launch %.3f ms = %.2f T "
              "pair-dimensions/s | f2v_silhouette %.3f ms = %.2f T pair-dimensions/s | rank / silhouette time %.2f" % (
                  args.small_scale, n, args.dim, block, t_xx * 1e3, t_nn * 1e3, rank * 1e3, pd / rank * 1e-12, t_sil * 1e3, pd / t_sil * 1e-12, rank / t_sil), flush=True)
    eng.set_param("trust_block", 0)
    y = eng.pca(2)
    t = median(lambda: eng.trustworthiness(y, 5, ids).seconds, args.reps)[0]
    print("RMAT-%d: f2v_trustworthiness of the PCA layout (d2 = 2), 8192 samples: %.3f ms" % (args.small_scale, t * 1e3), flush=True)
    eng.close()

    # 3. cora, every vertex
    rowptr, colids = F.read_mtx(args.cora)
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 200, 256, 5, 0.02)
    p = eng.pca(2, details=True)
    t_pca = median(lambda: eng.pca(2, details=True).info.seconds, args.reps)[0]
    res = eng.trustworthiness(p.y, 5)
    t = median(lambda: eng.trustworthiness(p.y, 5).seconds, args.reps)[0]
    print("cora n=%d D=%d after 200 epochs: f2v_pca(2) %.3f ms (%d sweeps), f2v_trustworthiness of it, every vertex, k=5: %.3f ms (trustworthiness %.4f continuity %.4f "
          "overlap %.4f)" % (len(rowptr) - 1, args.dim, t_pca * 1e3, p.info.sweeps, t * 1e3, res.trustworthiness, res.continuity, res.overlap), flush=True)
    eng.close()

    # 1. and 4. the large graph
    rowptr, colids = rmat_csr(args.scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 3, 65536, 5, 0.02)
    p = eng.pca(2, details=True)
    t_pca, t_min = median(lambda: eng.pca(2, details=True).info.seconds, args.reps)
    floor = n * args.dim * 4 / (gbps.value * 1e9)
    print("RMAT-%d n=%d D=%d: f2v_pca(2) %.3f ms (min %.3f, %d sweeps) | one read of the matrix at the copy rate %.3f ms: %.1f x | scatter matrix: %.2f T fp64 fma/s" % (
        args.scale, n, args.dim, t_pca * 1e3, t_min * 1e3, p.info.sweeps, floor * 1e3, t_pca / floor, n * args.dim * (args.dim + 64) / 2 / t_pca * 1e-12), flush=True)
    ids = np.random.default_rng(1).permutation(n)[:4096].astype(np.uint32)
    res = eng.trustworthiness(p.y, 5, ids)
    t = median(lambda: eng.trustworthiness(p.y, 5, ids).seconds, args.reps)[0]
    print("RMAT-%d: f2v_trustworthiness of the PCA layout, 4096 samples, k=5: %.3f ms (trustworthiness %.4f continuity %.4f overlap %.4f); every vertex would take %.0f s" % (
        args.scale, t * 1e3, res.trustworthiness, res.continuity, res.overlap, t * n / 4096), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
