#!/usr/bin/env python3
"""Time the GPU t-SNE layout (include/f2v.h: t-SNE layout) at m = 2708 (cora's size), 16384 and 65536 points, d2 = 2: the affinities,
a whole default call (1000 iterations from the PCA start) and the time of one iteration, from two calls on the same P and start that
differ only in their iteration count -- device time between events around the call's own launches, as the call reports it.  Pairs per
second are m^2 over the iteration time and are compared with what the vector ALUs could issue: tsne_pair_kernel's loop compiles to 153
vector instructions per 8 pairs at d2 = 2 (hipcc -S for gfx950: 11 of the 19 per pair are the correctly rounded division), and a CU
issues one 64-lane vector instruction per SIMD every two clocks -- 256 CUs x 4 SIMDs x 2.4 GHz / 2 x 64 lanes = 78.6 T lane-instructions/s,
the rate behind the 157.3 TFLOP/s fp32 vector peak.  An iteration also holds the Z reduction and the step kernel; the kernel split is

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/tsne_time.py --profile-pass 16384

    python tools/tsne_time.py > profiles/tsne_time.txt

The points are 16 Gaussian clusters in 32 dimensions on a ring graph (the layout reads the matrix alone).  For scale: scikit-learn's
TSNE(method="exact") took 13 s for 600 points on the CPU of the machine the tests were written on."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import force2vec_amd as F  # noqa: E402

VALU_PER_PAIR = 153 / 8.0
LANE_INSTRUCTIONS = 256 * 4 * 2.4e9 / 2 * 64


def engine(m, D=32, seed=1):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((16, D))[rng.integers(0, 16, m)] + 0.45 * rng.standard_normal((m, D))).astype(np.float32)
    v = np.arange(m)
    nb = np.sort(np.stack([(v - 1) % m, (v + 1) % m], axis=1), axis=1)
    eng = F.Engine((2 * np.arange(m + 1)).astype(np.uint32), nb.reshape(-1).astype(np.uint32), D)
    eng.set_embeddings(X)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2708, 16384, 65536])
    ap.add_argument("--profile-pass", type=int, default=0, metavar="M", help="200 iterations at M points and nothing else (run under rocprofv3)")
    args = ap.parse_args()
    if args.profile_pass:
        eng = engine(args.profile_pass)
        eng.tsne(2, iters=200)
        eng.close()
        return
    floor = LANE_INSTRUCTIONS / VALU_PER_PAIR
    print("vector-issue bound: %.1f T lane-instructions/s / %.1f instructions per pair = %.2f T pairs/s" % (LANE_INSTRUCTIONS * 1e-12, VALU_PER_PAIR, floor * 1e-12), flush=True)
    for m in args.sizes:
        eng = engine(m)
        t0 = time.perf_counter()
        P = eng.tsne_affinities(30.0)
        t_aff, wall_aff = eng.last_layout_seconds, time.perf_counter() - t0
        y0 = 1e-4 * np.random.default_rng(2).standard_normal((m, 2))
        eng.tsne(2, iters=20, P=P, init=y0)  # warm: code objects, workspace
        short, long_ = 50, 250
        a = min(eng.tsne(2, iters=short, P=P, init=y0, details=True)[1]["seconds"] for _ in range(3))
        b = min(eng.tsne(2, iters=long_, P=P, init=y0, details=True)[1]["seconds"] for _ in range(3))
        per = (b - a) / (long_ - short)
        t0 = time.perf_counter()
        y, info = eng.tsne(2, details=True)
        wall = time.perf_counter() - t0
        trust = eng.trustworthiness(y, 5, ids=np.random.default_rng(3).permutation(m)[:2048].astype(np.uint32)).trustworthiness
        print("m=%d: affinities %.3f ms on the device (%.3f s with the host's symmetric sum), %d nonzeros | one iteration %.3f ms = %.3f T pairs/s = %.0f %% of the "
              "vector-issue bound | the default call (1000 iterations, PCA start, affinities included): %.3f s on the device, %.3f s wall, KL %.4f, trustworthiness "
              "(k = 5, 2048 samples) %.4f" % (m, t_aff * 1e3, wall_aff, len(P[1]), per * 1e3, m * m / per * 1e-12, 100.0 * m * m / per / floor, info["seconds"], wall,
                                                info["kl"], trust), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
