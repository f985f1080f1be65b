#!/usr/bin/env python3
"""Time the three held-out link-prediction calls (include/f2v.h: f2v_edge_split, f2v_pair_scores, f2v_ranking).

    python tools/heldout_time.py [--scale 20] [--dim 128] [--frac 0.2] [--ratio 1] [--reps 3] [--pairs 16777216] [--pairs-only]
        > profiles/heldout_time.txt

The split of an RMAT graph (count-only call, filling call, what the anchor rule leaves of frac -- also on cora), then on the
training graph's engine (one epoch of option 5: the time is what is measured) the pair scores of the held-out set and of `--pairs`
uniformly random pairs per metric -- rows gathered per second beside the random-row gather rates of this box that bench.py reports
(f2v_diag_gather_rate) -- and the ranking of both sets.  --pairs-only stops after the pair scores of the random pairs: with
F2V_LIBRARY naming another build of the library it times that build's kernel layout."""
import argparse
import ctypes as C
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


def median_of(call, reps):
    """-> (median of call()'s value over `reps` runs after one warm-up, the last value)"""
    vals = [call() for _ in range(reps + 1)][1:]
    return statistics.median(vals), vals[-1]


def split_line(name, info):
    print("%s: %d edges, %d candidates (%.4f of the edges), %d protected by an anchor, %d held: share %.4f; training nnz %d, %d negatives, %d drawn, %d capped" % (
        name, info.edges, info.candidates_held, info.candidates_held / max(info.edges, 1), info.protected, info.held, info.held / max(info.edges, 1),
        info.train_nnz, info.negatives, info.drawn, info.capped), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--frac", type=float, default=0.2)
    ap.add_argument("--ratio", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1 << 24)
    ap.add_argument("--pairs-only", action="store_true")
    a = ap.parse_args()
    rowptr, colids = rmat_csr(a.scale)
    n = len(rowptr) - 1
    print("library: %s" % os.environ.get("F2V_LIBRARY", _lib.LIB_PATH), flush=True)
    print("RMAT scale %d: n = %d, nnz = %d; D = %d" % (a.scale, n, len(colids), a.dim), flush=True)
    full = F.Engine(rowptr, colids, 4)

    def count_only():
        c, info = [C.c_uint64() for _ in range(3)], _lib.SplitInfo()
        _lib.check(full._L.f2v_edge_split(full._h, a.frac, 1, a.ratio, None, None, 0, None, None, 0, None, None, 0, *[C.byref(x) for x in c], C.byref(info)), full._L)
        return info.seconds

    tc, _ = median_of(count_only, a.reps)
    walls = []

    def whole():
        t = time.perf_counter()
        s = whole.last = full.edge_split(frac=a.frac, seed=1, ratio=a.ratio, details=True)
        walls.append(time.perf_counter() - t)
        return s.info.seconds

    dev, _ = median_of(whole, a.reps)
    split = whole.last
    print("f2v_edge_split(frac %g, ratio %d): count-only call %.3f ms on the device (anchors, decisions, three prefix sums); filling call %.3f ms (fill, negatives); "
          "Engine.edge_split %.1f ms wall" % (a.frac, a.ratio, tc * 1e3, (dev - tc) * 1e3, statistics.median(walls[1:]) * 1e3), flush=True)
    split_line("RMAT-%d frac %g" % (a.scale, a.frac), split.info)
    if not a.pairs_only:
        for frac in (0.1, 0.3, 0.5):
            split_line("RMAT-%d frac %g" % (a.scale, frac), full.edge_split(frac=frac, seed=1, ratio=a.ratio, details=True).info)
        cr, cc = F.read_mtx(os.path.join(ROOT, "tests", "golden", "cora.mtx"))
        cora = F.Engine(cr, cc, 4)
        for frac in (0.1, 0.2, 0.3, 0.5):
            split_line("cora frac %g" % frac, cora.edge_split(frac=frac, seed=1, ratio=a.ratio, details=True).info)
        cora.close()
    full.close()

    eng = F.Engine(split.rowptr, split.colids, a.dim)
    eng.srand(1)
    eng.init_embeddings(_lib.INIT_SYMMETRIC)
    eng.train(5, 1, 65536)
    g = C.c_double()
    for name, table in (("4-GiB table (the bench line's row_gather_from_hbm)", 4 << 30), ("table of the matrix's size", n * a.dim * 4), ("64-MiB table (infinity cache)", 64 << 20)):
        if eng._L.f2v_diag_gather_rate(0, table, 2, C.byref(g)) == 0:
            print("random-row gather rate of this box, %s: %.0f GB/s = %.3g rows of %d B per second" % (name, g.value, g.value * 1e9 / 512, 512), flush=True)
    rng = np.random.default_rng(1)
    sets = [("held-out set", np.concatenate([split.held_u, split.neg_u]), np.concatenate([split.held_v, split.neg_v]),
             np.concatenate([np.ones(len(split.held_u), dtype=np.uint8), np.zeros(len(split.neg_u), dtype=np.uint8)])),
            ("uniformly random pairs", rng.integers(0, n, a.pairs).astype(np.uint32), rng.integers(0, n, a.pairs).astype(np.uint32), (rng.random(a.pairs) < 0.5).astype(np.uint8))]
    for name, u, v, y in sets:
        m = len(u)
        for metric in ("dot", "l2", "cos"):
            walls = []

            def scores():
                t = time.perf_counter()
                scores.last = eng.pair_scores(u, v, metric)
                walls.append(time.perf_counter() - t)
                return eng.last_pairs_seconds

            dev, _ = median_of(scores, a.reps)
            print("f2v_pair_scores, %s (%d pairs), %s: %.3f ms on the device = %.3g rows gathered per second = %.0f GB/s of rows; %.1f ms wall (\"pairs_chunk\" %d)" % (
                name, m, metric, dev * 1e3, 2 * m / dev, 2 * m * a.dim * 4 / dev * 1e-9, statistics.median(walls[1:]) * 1e3, eng.get_param("pairs_chunk")), flush=True)
        if a.pairs_only:
            continue
        s = scores.last.astype(np.float64)
        walls = []

        def rank():
            t = time.perf_counter()
            rank.last = eng.ranking(s, y)
            walls.append(time.perf_counter() - t)
            return rank.last.seconds

        dev, _ = median_of(rank, a.reps)
        r = rank.last
        print("f2v_ranking, %s (%d items, %d groups): %.3f ms on the device = %.3g items per second; %.1f ms wall; AUC %.6f AP %.6f" % (
            name, m, r.groups, dev * 1e3, m / dev, statistics.median(walls[1:]) * 1e3, r.auc, r.ap), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
