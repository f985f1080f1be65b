#!/usr/bin/env python3
"""Time the component calls (include/f2v.h: f2v_components, f2v_spanning_forest, f2v_edge_split_connected, f2v_subgraph).

    python tools/components_time.py [--scale 20] [--frac 0.2] [--ratio 1] [--reps 3] > profiles/components_time.txt

On an RMAT graph: device time and rounds of the components and of both spanning forests with the host's wall time of every Boruvka
round, the connected split beside the anchor split timed in the same run (every repetition of the connected split takes a seed of its
own: the handle keeps the forest of the last seed), the subgraph of the largest component, and what the two rules hold of frac."""
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
    ap.add_argument("--frac", type=float, default=0.2)
    ap.add_argument("--ratio", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rowptr, colids = rmat_csr(a.scale)
    n = len(rowptr) - 1
    print("library: %s" % os.environ.get("F2V_LIBRARY", _lib.LIB_PATH), flush=True)
    print("RMAT scale %d: n = %d, nnz = %d, longest row %d, rows longer than 256 nonzeros: %d" % (
        a.scale, n, len(colids), int(np.diff(rowptr.astype(np.int64)).max()), int((np.diff(rowptr.astype(np.int64)) > 256).sum())), flush=True)
    eng = F.Engine(rowptr, colids, 4)

    secs = []
    for _ in range(a.reps + 1):
        labels, info = eng.components(details=True)
        secs.append(info.seconds)
    print("f2v_components: %.3f ms on the device, %d rounds: %d components, %d isolated, largest %d (label %d), %d distinct pairs" % (
        statistics.median(secs[1:]) * 1e3, info.rounds, info.components, info.isolated, info.largest, info.largest_label, info.edges), flush=True)

    for greatest in (True, False):
        secs, walls = [], []
        for _ in range(a.reps + 1):
            t = time.perf_counter()
            u, v, f = eng.spanning_forest(seed=1, greatest=greatest, details=True)
            walls.append(time.perf_counter() - t)
            secs.append(f.seconds)
        print("f2v_spanning_forest(%s): %.3f ms on the device, %.1f ms wall, %d rounds, %d pairs, %d components" % (
            "greatest" if greatest else "least", statistics.median(secs[1:]) * 1e3, statistics.median(walls[1:]) * 1e3, f.rounds, f.forest_edges, f.components), flush=True)
        print("    host wall time per round (every round scans all nonzeros twice; the last finds nothing), ms: %s" % " ".join("%.3f" % (s * 1e3) for s in f.round_seconds), flush=True)

    def split(keep, seed):
        t = time.perf_counter()
        s = eng.edge_split(frac=a.frac, seed=seed, ratio=a.ratio, details=True, keep=keep)
        return s, time.perf_counter() - t

    for keep in ("anchor", "forest"):
        runs = [split(keep, 1 + rep if keep == "forest" else 1) for rep in range(a.reps + 1)][1:]
        s = split(keep, 1)[0]
        print("Engine.edge_split(frac %g, ratio %d, keep=%s): %.3f ms on the device (count-only and filling call together%s), %.1f ms wall" % (
            a.frac, a.ratio, keep, statistics.median([r[0].info.seconds for r in runs]) * 1e3, "; the forest and its flags included" if keep == "forest" else "",
            statistics.median([r[1] for r in runs]) * 1e3), flush=True)
        print("    seed 1: %d edges, %d candidates, %d protected, %d held: share %.4f of the edges; training nnz %d, %d negatives" % (
            s.info.edges, s.info.candidates_held, s.info.protected, s.info.held, s.info.held / max(s.info.edges, 1), s.info.train_nnz, s.info.negatives), flush=True)

    secs, walls = [], []
    for _ in range(a.reps + 1):
        t = time.perf_counter()
        sub = eng.subgraph(labels == info.largest_label)
        walls.append(time.perf_counter() - t)
        secs.append(eng.last_subgraph_seconds)
    print("f2v_subgraph(largest component): %.3f ms on the device (count-only and filling call's launches), %.1f ms wall: %d rows, %d nonzeros" % (
        statistics.median(secs[1:]) * 1e3, statistics.median(walls[1:]) * 1e3, len(sub.ids), len(sub.colids)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
