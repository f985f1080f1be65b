#!/usr/bin/env python3
"""Time the GPU build of the link-prediction pair set (include/f2v.h: f2v_link_pairs) and the score that uses it.

    python tools/linkpairs_time.py [--scale 20] [--dim 128] [--ratio 2] [--reps 3] [--short 0 64 128 256 512 1024] [--no-score]
        > profiles/linkpairs_time.txt

Per value of "link_short_max": the device seconds of the count-only call (the counts and the prefix sums) and of the filling call
(the negatives, the positives and their scattered stores), and the wall time of Engine.link_pairs.  Then the vertex with the most
negatives alone (the same graph with every other row emptied: its candidates are the same), the wall time of Engine.link_predict()
with its parts, and tests/linkpred_harness.pair_set on cora on the host for context.  A run under `rocprofv3 --kernel-trace --stats`
with --no-score splits the filling call by kernel."""
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


def timed_pairs(eng, ratio, reps):
    """-> (median device seconds of the whole Engine.link_pairs, median wall seconds, the last result)"""
    dev, wall = [], []
    for rep in range(reps + 1):  # the first call is the warm-up: workspace, code objects
        t = time.perf_counter()
        out = eng.link_pairs(ratio=ratio, seed=1, details=True)
        if rep:
            wall.append(time.perf_counter() - t)
            dev.append(out[3].seconds)
    return statistics.median(dev), statistics.median(wall), out


def count_seconds(eng, ratio, reps):
    import ctypes as C
    secs = []
    for rep in range(reps + 1):
        count, info = C.c_uint64(), _lib.LinkInfo()
        _lib.check(eng._L.f2v_link_pairs(eng._h, ratio, 1, None, None, None, 0, C.byref(count), C.byref(info)), eng._L)
        if rep:
            secs.append(info.seconds)
    return statistics.median(secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--ratio", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--short", type=int, nargs="+", default=[0, 64, 128, 256, 512, 1024])
    ap.add_argument("--no-score", action="store_true")
    a = ap.parse_args()
    rowptr, colids = rmat_csr(a.scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, a.dim)
    default = eng.get_param("link_short_max")
    print("RMAT scale %d: n = %d, nnz = %d; ratio %d; \"link_short_max\" defaults to %d" % (a.scale, n, len(colids), a.ratio, default), flush=True)
    tc = count_seconds(eng, a.ratio, a.reps)
    print("count-only call (counts, prefix sums): %.3f ms" % (tc * 1e3), flush=True)
    first = None
    for short in a.short + [default]:
        eng.set_param("link_short_max", short)
        dev, wall, out = timed_pairs(eng, a.ratio, a.reps)
        u, v, y, info = out
        if first is None:
            first = out
            print("M = %d: %d positives, %d negatives, %d candidates (%.4f per negative), %d vertices capped" % (
                len(y), info.positives, info.negatives, info.candidates, info.candidates / max(info.negatives, 1), info.capped), flush=True)
        equal = all(np.array_equal(g, w) for g, w in zip(out[:3], first[:3]))
        print("\"link_short_max\" = %4d: filling call %.3f ms on the device (Engine.link_pairs: both calls %.3f ms on the device, %.1f ms wall); result %s" % (
            short, (dev - tc) * 1e3, dev * 1e3, wall * 1e3, "equal to the first" if equal else "DIFFERENT"), flush=True)
    # the vertex with the most negatives alone
    negs = np.bincount(first[0][first[2] == 0], minlength=n)
    big = int(np.argmax(negs))
    lone_rowptr = np.zeros(n + 1, dtype=np.uint32)
    lone_rowptr[big + 1:] = rowptr[big + 1] - rowptr[big]
    lone = F.Engine(lone_rowptr, np.ascontiguousarray(colids[rowptr[big]:rowptr[big + 1]]), 4)
    tcl = count_seconds(lone, a.ratio, a.reps)
    dev, wall, out = timed_pairs(lone, a.ratio, a.reps)
    print("vertex %d alone (%d nonzeros, %d negatives, %d candidates): filling call %.3f ms on the device" % (
        big, rowptr[big + 1] - rowptr[big], out[3].negatives, out[3].candidates, (dev - tcl) * 1e3), flush=True)
    lone.close()
    if not a.no_score:
        eng.srand(1)
        eng.init_embeddings(_lib.INIT_UNIT)
        eng.train(6, 2, 65536)
        for rep in range(2):
            t0 = time.perf_counter()
            u, v, y = eng.link_pairs(ratio=a.ratio, seed=1)
            t1 = time.perf_counter()
            cv = len(y) // 2
            model = eng.logreg_fit(pairs=(u[:cv], v[:cv]), y=y[:cv].reshape(-1, 1))
            t2 = time.perf_counter()
            z = eng.logreg_decision(model, pairs=(u[cv:], v[cv:]))
            t3 = time.perf_counter()
            print("the parts of Engine.link_predict() at D = %d, run %d: pairs %.3f s, fit %.3f s (%.3f s on the device, %d iterations, %d evaluations), decision %.3f s (%.3f s on the device)" % (
                a.dim, rep, t1 - t0, t2 - t1, model.seconds, model.iterations[0], model.evaluations[0], t3 - t2, eng.last_logreg_seconds), flush=True)
        t0 = time.perf_counter()
        scores = eng.link_predict(ratio=a.ratio, seed=1)
        print("Engine.link_predict(): %.3f s wall; accuracy %.3f F1-macro %.3f F1-micro %.3f (two epochs of option 6: the time is what is measured)" % (
            (time.perf_counter() - t0,) + tuple(scores)), flush=True)
    eng.close()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import linkpred_harness as LP
    cr, cc = F.read_mtx(os.path.join(ROOT, "tests", "golden", "cora.mtx"))
    t0 = time.perf_counter()
    pairs = LP.pair_set(cr, cc, seed=0)
    t = time.perf_counter() - t0
    print("for context, tests/linkpred_harness.pair_set on cora on the host: %d pairs in %.1f ms = %.0f pairs/s (a Python loop with a set per vertex)" % (
        len(pairs[2]), t * 1e3, len(pairs[2]) / t), flush=True)


if __name__ == "__main__":
    main()
