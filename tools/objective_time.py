#!/usr/bin/env python3
"""Time of one evaluation of the training objective (f2v_objective) against one training epoch, in the same process.

Headline: RMAT-20 (bench.py's graph), D = 128, ns = 5, options 5 and 6, warm.  Device time of both from HIP events: f2v_train with
"loss_every" = 1 brackets its evaluation with events ("last_loss_us") and reports the epoch alone (seconds_out).  Also the host
wall time of a synchronous f2v_objective call, the bytes it gathers per second against the on-box row-gather ceilings
(f2v_diag_gather_rate), and cora at 1200 epochs with "loss_every" 1 against 0.
  python tools/objective_time.py [--reps R] [--quick]      (--quick: the headline only, fewer reps: for a rocprofv3 run)"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
import force2vec_amd as F
from force2vec_amd import _lib


def headline(option, reps):
    rowptr, colids = bench.load_graph(20, 16, 1)
    n, nnz, D, ns = len(rowptr) - 1, int(rowptr[-1]), 128, 5
    eng = F.Engine(rowptr, colids, D)
    eng.srand(1)
    eng.init_embeddings(0 if option == 5 else 1)
    eng.train(option, 2, 65536)  # plans, warm-up
    eng.objective(option, ns)
    eng.set_param("loss_every", 1)
    epoch_ms, eval_ms = [], []
    for _ in range(reps):
        epoch_ms.append(eng.train(option, 1, 65536, ns) * 1e3)
        eval_ms.append(eng.get_param("last_loss_us") * 1e-3)
    eng.set_param("loss_every", 0)
    host_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        o = eng.objective(option, ns)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert o.positive_pairs == nnz and o.negative_pairs == n * ns
    eng.close()
    # bytes the evaluation must gather: one row per pair and per item's x_i (pieces of <= 64 neighbours), 4 B per neighbour id
    items = int(np.sum(np.maximum(1, (np.diff(rowptr.astype(np.int64)) + 63) // 64)))
    gathered = (nnz + n * ns + items) * 4 * D + nnz * 4
    med_eval, med_epoch = float(np.median(eval_ms)), float(np.median(epoch_ms))
    return {"graph": "rmat20", "option": option, "n": n, "nnz": nnz, "D": D, "ns": ns, "reps": reps,
            "epoch_ms_median": round(med_epoch, 4), "epoch_ms_min": round(min(epoch_ms), 4),
            "objective_ms_median": round(med_eval, 4), "objective_ms_min": round(min(eval_ms), 4),
            "objective_over_epoch": round(med_eval / med_epoch, 3),
            "objective_host_call_ms_median": round(float(np.median(host_ms)), 4),
            "objective_gathered_bytes": gathered, "objective_GBs": round(gathered / (med_eval * 1e-3) * 1e-9, 1)}


def gather_ceilings():
    L = _lib.lib()
    out = {}
    for name, size in (("gather_GBs_4GiB_table", 4 << 30), ("gather_GBs_512MiB_table", 512 << 20), ("gather_GBs_64MiB_table", 64 << 20)):
        g = ctypes.c_double()
        if L.f2v_diag_gather_rate(0, size, 2, ctypes.byref(g)) == 0:
            out[name] = round(g.value, 1)
    return out


def cora_overhead():
    rowptr, colids = F.read_mtx(os.path.join(ROOT, "tests", "golden", "cora.mtx"))
    res = {}
    for k in (0, 1, 0, 1):  # twice each, the second pair counted (warm)
        eng = F.Engine(rowptr, colids, 128)
        eng.srand(1)
        eng.init_embeddings(0)
        eng.set_param("loss_every", k)
        t0 = time.perf_counter()
        sec = eng.train(5, 1200, 384)
        wall = time.perf_counter() - t0
        res["loss_every_%d" % k] = {"epoch_loop_s": round(sec, 5), "wall_s": round(wall, 4), "last_loss_us": eng.get_param("last_loss_us"),
                                    "last_wide_epochs": eng.get_param("last_wide_epochs"), "entries": len(eng.train_losses()[0])}
        eng.close()
    a, b = res["loss_every_0"], res["loss_every_1"]
    res["wall_overhead"] = round(b["wall_s"] / a["wall_s"] - 1.0, 3)
    res["device_overhead"] = round((b["epoch_loop_s"] + b["last_loss_us"] * 1e-6) / a["epoch_loop_s"] - 1.0, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"headline": [headline(o, 5 if args.quick else args.reps) for o in ((5,) if args.quick else (5, 6))]}
    if not args.quick:
        out["gather_ceilings"] = gather_ceilings()
        out["cora_1200_epochs"] = cora_overhead()
    print(json.dumps(out, indent=1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
