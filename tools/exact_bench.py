#!/usr/bin/env python3
"""Time of the exact all-pairs Force2Vec (option 1) and of its objective, device time from HIP events.

cora (B = 256 and B = n) and seeded RMAT graphs of scale 15 and 16 (B = 384 and 16384), D = 128: ms per epoch, pair-dimensions per
second (n x n x D per epoch), and the share of the MI355X's 157.3 TFLOPS fp32 vector peak the pair kernel reaches, counting the
definition's operations per pair-dimension: the subtraction, the square, the tree's addition, the product with the coefficient, the
two comparisons of scale(), the product with STEP and the addition onto the piece sum -- 8 (the fp64 coefficient, one per pair,
is not counted).  Then the exact objective on the same graphs, and the genuine reference binary (oracle/_ref/Force2Vec -option 1,
where it was built) on cora on this machine's host cores with 16 threads, 48 epochs.  Every training figure is taken three times: with the
engine's own choice of the pair kernel ("default"), and with the quarter-wave and the generic-layout kernel pinned.
  python tools/exact_bench.py [--quick] > profiles/exact_time.txt      (--quick: cora and scale 15 only)"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
import force2vec_amd as F

PEAK_FP32_VECTOR = 157.3e12
OPS_PER_PAIR_DIM = 8
D = 128
KERNELS = [("default", ()), ("quarter-wave", (("exact_quarter_min", 0),)), ("generic", (("quarter_wave", 0),))]


def measure(name, rowptr, colids, batches, epochs):
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    eng = F.Engine(rowptr, colids, D)
    out = []
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        X0 = eng.get_embeddings()
        # the engine's own choice of the pair kernel, then each of the two kernels pinned (they give the same bits)
        for batch, (kernel, params) in [(b, k) for b in batches for k in KERNELS]:
            for k, v in (("quarter_wave", 1), ("exact_quarter_min", 1024)) + params:
                eng.set_param(k, v)
            eng.set_embeddings(X0)
            eng.set_param("exact_epoch", 0)
            eng.train(1, 1, batch)  # warm-up: the workspace is allocated here
            ms = [eng.train(1, 1, batch) * 1e3 for _ in range(epochs)]
            med = float(np.median(ms))
            pd = float(n) * n * D
            out.append({"graph": name, "n": n, "nnz": nnz, "D": D, "batch": min(batch, n), "kernel": kernel,
                        "ran_quarter_wave": eng.get_param("last_exact_quarter"), "exact_rows": eng.get_param("last_exact_rows"), "epochs_timed": epochs,
                        "epoch_ms_median": round(med, 3), "epoch_ms_min": round(min(ms), 3),
                        "pair_dims_per_s": float("%.4g" % (pd / (med * 1e-3))),
                        "share_of_fp32_vector_peak": round(pd * OPS_PER_PAIR_DIM / (med * 1e-3) / PEAK_FP32_VECTOR, 4)})
        for k, v in (("quarter_wave", 1), ("exact_quarter_min", 1024)):
            eng.set_param(k, v)
        eng.objective(1)  # warm-up
        eng.set_param("loss_every", 1)
        ms = []
        for _ in range(max(2, epochs)):
            eng.train(1, 1, batches[-1])
            ms.append(eng.get_param("last_loss_us") * 1e-3)
        eng.set_param("loss_every", 0)
        o = eng.objective(1)
        out.append({"graph": name, "n": n, "D": D, "objective_ms_median": round(float(np.median(ms)), 3), "objective_ms_min": round(min(ms), 3),
                    "pair_dims_per_s": float("%.4g" % (float(n) * n * D / (float(np.median(ms)) * 1e-3))), "loss": o.loss,
                    "negative_pairs": o.negative_pairs})
    finally:
        eng.close()
    return out


def reference_on_cora(threads=16, iters=48):  # (the reference prints a float: its timer shows steps of 1/64 s)
    from oracle import oracle as O
    if O.ref_binary() is None:
        return {"reference": "oracle/_ref/Force2Vec was not built here"}
    with tempfile.TemporaryDirectory() as td:
        _, out = O.run_reference(os.path.join(ROOT, "tests", "golden", "cora.mtx"), td, 1, iters, 256, D, threads=threads)
    sec = [float(l.split(":")[1].split()[0]) for l in out.splitlines() if l.startswith("Force2Vec Parallel Wall time required:")]
    return {"reference": "oracle/_ref/Force2Vec -option 1 -threads %d on cora, B = 256, D = %d" % (threads, D), "epochs": iters,
            "wall_seconds": sec[0] if sec else None, "epoch_ms": round(sec[0] / iters * 1e3, 1) if sec else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    rowptr, colids = F.read_mtx(os.path.join(ROOT, "tests", "golden", "cora.mtx"))
    for r in measure("cora", rowptr, colids, [256, len(rowptr) - 1], 5):
        print(json.dumps(r), flush=True)
    for scale in (15,) if args.quick else (15, 16):
        rowptr, colids = bench.load_graph(scale, 16, 1)
        for r in measure("rmat%d" % scale, rowptr, colids, [384, 16384], 3 if scale == 15 else 2):
            print(json.dumps(r), flush=True)
    print(json.dumps(reference_on_cora()), flush=True)


if __name__ == "__main__":
    main()
