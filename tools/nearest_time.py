#!/usr/bin/env python3
"""Time the nearest-neighbour queries (include/f2v.h) on an RMAT graph: each metric at nq = 1 / 1024 / 65536 and the all-vertices
sweep for dot, warm, device time from seconds_out; next to them the expression a user would otherwise write,
`(X[q] @ X.T).topk(k)` in query chunks that fit memory, timed with events, interleaved with the library's calls rep by rep.

    python tools/nearest_time.py [--scale 20] [--dim 128] [--k 10] > profiles/nearest_time.txt
    rocprofv3 --kernel-trace --stats -d /tmp/nn_prof -- python tools/nearest_time.py --profile-pass     # the kernel split

Reported per case: median and minimum time, pair-dimensions per second (nq * N * D / t) and, for dot, the fraction of the
157.3 TF fp32 matrix peak (2 flop per pair-dimension)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import force2vec_amd as F  # noqa: E402
from force2vec_amd.graph import rmat_csr  # noqa: E402

PEAK_TF = 157.3


def torch_topk(torch, Xt, q, k, chunk=4096):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = []
    for lo in range(0, len(q), chunk):
        out.append((Xt[q[lo:lo + chunk]] @ Xt.T).topk(k, dim=1).indices)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--profile-pass", action="store_true", help="two warm calls per metric at nq = 65536 and nothing else (run under rocprofv3)")
    args = ap.parse_args()
    torch = None
    if not (args.no_torch or args.profile_pass):
        import torch  # initialised before the engine: a process whose HIP runtime is already up shows torch no device
        try:
            torch.cuda.set_device(0)
            torch.zeros(1, device="cuda")
        except RuntimeError as e:
            print("# torch baseline left out: %s" % e)
            torch = None
    rowptr, colids = rmat_csr(args.scale)
    n = len(rowptr) - 1
    eng = F.Engine(rowptr, colids, args.dim)
    eng.srand(1)
    eng.init_embeddings(0)
    eng.train(5, 1, 65536, 5, 0.02)
    rng = np.random.default_rng(1)
    print("# RMAT-%d: n = %d, nnz = %d, D = %d, k = %d; one epoch of option 5" % (args.scale, n, eng.nnz, args.dim, args.k))
    if args.profile_pass:
        q = rng.choice(n, 65536, replace=False).astype(np.uint32)
        for metric in ("dot", "cos", "l2"):
            for _ in range(2):
                eng.nearest(ids=q, k=args.k, metric=metric)
            print("%s nq=65536: %.6f s" % (metric, eng.last_nearest_seconds))
        return
    Xt = torch.from_numpy(eng.get_embeddings()).cuda() if torch else None
    print("# case: median s (min s over reps) | pair-dims/s | fraction of %.1f TF (dot) | torch (X[q] @ X.T).topk(k): median s | library / torch" % PEAK_TF)
    for nq, reps in ((1, 10), (1024, 10), (65536, 3)):
        q = rng.choice(n, nq, replace=False).astype(np.uint32)
        qt = torch.from_numpy(q.astype(np.int64)).cuda() if torch else None
        for metric in ("dot", "cos", "l2"):
            eng.nearest(ids=q, k=args.k, metric=metric, exclude_self=False)  # warm-up (workspace, code objects)
            ours, theirs = [], []
            with_torch = torch is not None and metric == "dot"
            if with_torch:
                torch_topk(torch, Xt, qt, args.k)
            for _ in range(reps):  # interleaved: both see the same clocks
                ids, _ = eng.nearest(ids=q, k=args.k, metric=metric, exclude_self=False)
                ours.append(eng.last_nearest_seconds)
                if with_torch:
                    t, out = torch_topk(torch, Xt, qt, args.k)
                    theirs.append(t)
            t = statistics.median(ours)
            line = "%-4s nq=%-6d %.6f s (min %.6f, %d reps) | %.3e pair-dims/s" % (metric, nq, t, min(ours), reps, nq * n * args.dim / t)
            if metric == "dot":
                line += " | %.3f of peak" % (2.0 * nq * n * args.dim / t / (PEAK_TF * 1e12))
            if with_torch:
                tt = statistics.median(theirs)
                agree = float((torch.cat(out).cpu().numpy() == ids.astype(np.int64)).mean())
                line += " | torch %.6f s | %.2f x torch's time (ids agree on %.4f of the slots: torch's scores are not the fmaf chain)" % (tt, t / tt, agree)
            print(line, flush=True)
    if not args.no_sweep:
        eng.nearest(k=args.k, metric="dot")
        t = eng.last_nearest_seconds
        print("dot  all %d vertices: %.3f s | %.3e pair-dims/s | %.3f of peak" % (n, t, n * n * args.dim / t, 2.0 * n * n * args.dim / t / (PEAK_TF * 1e12)), flush=True)
        hits, possible = eng.neighbour_recall(args.k, "dot")
        print("neighbour_recall(dot, all): %d / %d in %.3f s" % (hits, possible, eng.last_nearest_seconds))
    eng.close()


if __name__ == "__main__":
    main()
