#!/usr/bin/env python3
"""Time the communities of the graph on the GPU (include/f2v.h: f2v_louvain) and the agreement of two labellings.

    python tools/louvain_time.py [--scale 20] [--reps 3] [--no-cora] > profiles/louvain_time.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/louvain_time.py --profile-pass     # the kernel split

Warm, median of --reps: the whole call; per level its nodes, communities and sweeps with the device time it adds (the call with
max_levels = l + 1 less the call with max_levels = l); level 0 under the placements of "louvain_short_max" / "louvain_lds_slots" (all
tables of short rows in workgroups' LDS instead of 16 lanes'; no table in LDS).  (A call with fewer sweeps aggregates another
labelling, so a sweep is not the difference of two calls: the kernel split below gives it.)  Floors from the same process: one streaming read of the CSR plus a
4-byte gather per nonzero at the rates f2v_diag_stream_copy and f2v_diag_gather_rate report, and f2v_modularity's one pass over the
same nonzeros.  Then the agreement of the result with a random labelling, and on cora the wall time beside networkx's
louvain_communities on the host.  --profile-pass: two calls with max_levels = 1 and max_sweeps = --profile-sweeps (4) and nothing else -- four level-0 sweeps and
their aggregation each, the first call cold -- for a run under `rocprofv3 --kernel-trace --stats`, whose kernel_stats.csv splits a
sweep by kernel (the three move forms, apply, the two Qnum kernels)."""
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

EPOCH_MS = 1.84  # a training epoch of RMAT-20 at batch 65536


def timed(eng, reps, **kw):
    """-> (median device seconds, median wall seconds, the last result)"""
    dev, wall = [], []
    for rep in range(reps + 1):  # the first call is the warm-up: workspace, code objects
        t = time.perf_counter()
        out = eng.communities(details=True, **kw)
        if rep:
            wall.append(time.perf_counter() - t)
            dev.append(out[1].seconds)
    return statistics.median(dev), statistics.median(wall), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cora", action="store_true")
    ap.add_argument("--profile-pass", action="store_true", help="two truncated level-0 calls and nothing else (run under rocprofv3)")
    ap.add_argument("--profile-sweeps", type=int, default=4)
    a = ap.parse_args()
    rowptr, colids = rmat_csr(a.scale)
    n, nnz = len(rowptr) - 1, len(colids)
    eng = F.Engine(rowptr, colids, 4)
    print("RMAT scale %d: n = %d, nnz = %d, longest row %d; \"louvain_short_max\" = %d, \"louvain_lds_slots\" = %d" % (
        a.scale, n, nnz, int(np.diff(rowptr.astype(np.int64)).max()), eng.get_param("louvain_short_max"), eng.get_param("louvain_lds_slots")), flush=True)
    if a.profile_pass:
        for rep in range(2):
            _, info = eng.communities(max_levels=1, max_sweeps=a.profile_sweeps, details=True)
            print("call %d: %.3f ms on the device, %s" % (rep, info.seconds * 1e3, info.level_records), flush=True)
        eng.close()
        return
    dev, wall, (labels, info) = timed(eng, a.reps)
    print("whole call: %.2f ms on the device, %.2f ms wall = %.1f training epochs of %.2f ms; modularity %.6f, %d communities, %d levels, %d edges" % (
        dev * 1e3, wall * 1e3, dev * 1e3 / EPOCH_MS, EPOCH_MS, info.modularity, info.communities, info.levels, info.edges), flush=True)
    before = 0.0
    for l, rec in enumerate(info.level_records):
        d, _, _ = timed(eng, a.reps, max_levels=l + 1)
        took = d - before  # the difference of two medians of whole calls: a level of well under a millisecond is lost in their spread
        spent = "%.2f ms (%.3f ms per sweep, aggregation included)" % (took * 1e3, took * 1e3 / rec.sweeps) if took > 1e-3 else "below the resolution of a difference of two calls (1 ms)"
        print("level %d: %8d nodes -> %8d communities, %2d sweeps, %9d moves: %s" % (l, rec.nodes, rec.communities, rec.sweeps, rec.moves, spent), flush=True)
        before = max(before, d)
    level0, _, (_, info0) = timed(eng, a.reps, max_levels=1)
    sweep = level0 / info0.level_records[0].sweeps  # (an upper bound: prepare, placement and the aggregation are in it)
    for name, short_max, slots in (("every table of a short row in a workgroup's LDS", 0, 4096), ("no table in LDS above 16 lanes' rows", 32, 0),
                                   ("16 lanes up to 256 nonzeros", 256, 4096)):
        eng.set_param("louvain_short_max", short_max)
        eng.set_param("louvain_lds_slots", slots)
        t, _, (lab2, _) = timed(eng, a.reps, max_levels=1)
        print("  \"louvain_short_max\" = %3d, \"louvain_lds_slots\" = %4d (%s): level 0 %.2f ms against %.2f ms; result %s" % (
            short_max, slots, name, t * 1e3, level0 * 1e3, "equal" if np.array_equal(lab2, info.level_labels[0]) else "DIFFERENT"), flush=True)
    eng.set_param("louvain_short_max", 32)
    eng.set_param("louvain_lds_slots", 4096)
    copy, gather = C.c_double(), C.c_double()
    _lib.check(eng._L.f2v_diag_stream_copy(0, 1 << 30, 5, C.byref(copy)), eng._L)
    _lib.check(eng._L.f2v_diag_gather_rate(0, 32 << 20, 5, C.byref(gather)), eng._L)
    floor = (4.0 * (n + 1 + nnz)) / (copy.value * 1e9) + (4.0 * nnz) / (gather.value * 1e9)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        q = eng.modularity(labels, info.communities)
    mod = (time.perf_counter() - t0) / a.reps
    print("floors: stream copy %.0f GB/s, gather %.0f GB/s -> one read of the CSR and a 4-byte gather per nonzero %.3f ms: a level-0 sweep "
          "(level 0 over its sweeps, %.2f ms) is %.0f of them, and %.1f of modularity_kernel's 2.5 ms over the same nonzeros with a few clusters; "
          "Engine.modularity of the result (%d clusters, with its copies) %.2f ms wall" % (
              copy.value, gather.value, floor * 1e3, sweep * 1e3, sweep / floor, sweep * 1e3 / 2.5, info.communities, mod * 1e3), flush=True)
    assert q.q == info.modularity
    other = np.random.default_rng(1).integers(0, 50, n)
    t0 = time.perf_counter()
    ag = eng.agreement(labels, other)
    print("agreement with a random labelling of 50 clusters (%d x 50 cells): %.2f ms wall, %.3f ms on the device; NMI %.6f ARI %.6f" % (
        info.communities, (time.perf_counter() - t0) * 1e3, ag.seconds * 1e3, ag.nmi, ag.ari), flush=True)
    eng.close()
    if a.no_cora:
        return
    cr, cc = F.read_mtx(os.path.join(ROOT, "tests", "golden", "cora.mtx"))
    eng = F.Engine(cr, cc, 4)
    dev, wall, (labels, info) = timed(eng, a.reps)
    eng.close()
    print("cora: %.2f ms on the device, %.2f ms wall; modularity %.6f, %d communities, %d levels" % (dev * 1e3, wall * 1e3, info.modularity, info.communities, info.levels), flush=True)
    try:
        import networkx as nx
    except ImportError:
        print("networkx is not installed: no host comparison")
        return
    G = nx.Graph()
    G.add_nodes_from(range(len(cr) - 1))
    G.add_edges_from((u, int(v)) for u in range(len(cr) - 1) for v in cc[cr[u]:cr[u + 1]] if u < v)
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(G, seed=0)
    t = time.perf_counter() - t0
    print("for context, networkx louvain_communities on cora on the host: %.1f ms, modularity %.6f, %d communities" % (
        t * 1e3, nx.community.modularity(G, parts), len(parts)), flush=True)


if __name__ == "__main__":
    main()
