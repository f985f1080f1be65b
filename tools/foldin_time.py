#!/usr/bin/env python3
"""Time the GPU fold-in (include/f2v.h: f2v_fold_in): the plain form, whose every epoch gathers a vertex's list rows from the caches,
and -- with a build that has it: it measured slower and was taken out -- the resident form ("fold_resident" = 1),
which stages them once in LDS.

    python tools/foldin_time.py [--scale 20] [--dim 128] [--new 65536] [--iters 100] [--reps 3] [--cap 0] > profiles/foldin_time.txt

The matrix is an RMAT graph's after two epochs of training; the new vertices' lists are the CSR rows of `--new` existing vertices
chosen by a seeded permutation, so their lengths follow the graph's own degrees.  A call is stated as device seconds (events around
its launches) and as rows gathered per second -- info.pairs rows of D floats -- next to f2v_diag_gather_rate of the same process on a
table the size of the matrix and on one that fits an XCD's L2."""
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


def gather_rate(table_bytes):
    gbps = C.c_double()
    _lib.check(_lib.lib().f2v_diag_gather_rate(0, int(table_bytes), 5, C.byref(gbps)))
    return gbps.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--new", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--options", type=int, nargs="+", default=[5, 6])
    ap.add_argument("--cap", type=int, default=0, help="leave out the picked vertices whose lists are longer (0: none): the call's throughput without its longest serial chain")
    a = ap.parse_args()
    rowptr, colids = rmat_csr(a.scale)
    n = len(rowptr) - 1
    picked = np.random.RandomState(0).permutation(n)[:a.new]
    deg = (rowptr[picked + 1] - rowptr[picked]).astype(np.int64)
    if a.cap:
        picked, deg = picked[deg <= a.cap], deg[deg <= a.cap]
    q_rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint32)
    q_colids = np.concatenate([colids[rowptr[v]:rowptr[v + 1]] for v in picked]).astype(np.uint32)
    print("RMAT scale %d: n = %d, nnz = %d, D = %d; %d new vertices, %d list entries (longest %d, median %d), %d epochs, ns = 5" % (
        a.scale, n, len(colids), a.dim, len(picked), len(q_colids), deg.max(), int(np.median(deg)), a.iters), flush=True)
    row_bytes = a.dim * 4 + 4
    for name, table in (("the matrix's size", n * a.dim * 4), ("2 MiB (inside an XCD's L2)", 2 << 20)):
        g = gather_rate(table)
        print("f2v_diag_gather_rate, table of %s: %.0f GB/s = %.3g rows/s" % (name, g, g * 1e9 / row_bytes), flush=True)
    for option in a.options:
        eng = F.Engine(rowptr, colids, a.dim)
        eng.srand(1)
        eng.init_embeddings(_lib.INIT_SYMMETRIC if option == 5 else _lib.INIT_UNIT)
        eng.train(option, 2, 65536)
        results = {}
        for resident in (0, 1):
            try:
                eng.set_param("fold_resident", resident)
            except _lib.F2VError:
                print("option %d: \"fold_resident\" = %d is not available in this build" % (option, resident), flush=True)
                continue
            secs = []
            for rep in range(a.reps + 1):  # the first call is the warm-up: workspace, code objects
                y, info = eng.fold_in(q_rowptr, q_colids, option, a.iters, 5, 0.02, "mean", 1, details=True)
                if rep:
                    secs.append(info.seconds)
            results[resident] = y
            t = statistics.median(secs)
            print("option %d, \"fold_resident\" = %d (a resident launch ran: %s): %.2f ms per call (min %.2f of %d), %.3g rows/s gathered, %.0f GB/s of rows" % (
                option, resident, info.resident, t * 1e3, min(secs) * 1e3, a.reps, info.pairs / t, info.pairs * row_bytes / t * 1e-9), flush=True)
        if len(results) == 2:
            print("option %d: the two forms' results are %s" % (option, "bitwise equal" if np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32)) else "DIFFERENT"), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
