"""What the scorers share (the device buffers that grow on demand, the event timers, the entry preamble, the LDS
opt-in; f2v_separation.hip.h: sep_samples / sep_stage / sep_score).

Host test (no GPU): the compiled gfx950 code of the two kernels built from the shared device body, separation_pair_kernel and
trust_rank_kernel, both instantiations of each, both builds: no scratch, nothing spilled.  -m gpu: every family called on ONE handle,
interleaved, at a small size, then a large one, then the small one again -- every array and scalar must equal, bit for bit, the same
call on a fresh handle.  A buffer that was shrunk, shared between two families or not regrown shows there."""
import os
import subprocess

import numpy as np
import pytest

from test_gather_isa import FLAGS, HIPCC, function
from test_kmeans import engine_for, spills

gpu = pytest.mark.gpu

KERNELS = ["separation_pair_kernelILi64EE", "separation_pair_kernelILi128EE", "trust_rank_kernelILi64EE", "trust_rank_kernelILi128EE"]
TU = """#include "f2v_layout.hip.h"
template __global__ void f2v::separation_pair_kernel<64>(const f2v::SepPairArgs);
template __global__ void f2v::separation_pair_kernel<128>(const f2v::SepPairArgs);
template __global__ void f2v::trust_rank_kernel<64>(const f2v::TrustRankArgs);
template __global__ void f2v::trust_rank_kernel<128>(const f2v::TrustRankArgs);
"""


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")
@pytest.mark.parametrize("build", ["product", "selftest"])
def test_pair_and_rank_kernels_use_no_scratch_and_spill_nothing(tmp_path, build):
    src, out = str(tmp_path / "workspace_isa.hip"), str(tmp_path / "workspace_isa.s")
    with open(src, "w") as f:
        f.write(TU)
    defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
    subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(tmp_path), capture_output=True)
    text = open(out).read()
    for part in KERNELS:
        symbol, _ = function(text, part)
        assert ("selftest" in symbol) == (build == "selftest"), symbol  # the two builds keep distinct kernel symbols
        assert spills(text, symbol) == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (symbol, spills(text, symbol))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
N, D = 1500, 40  # D: a multiple of 4 but not of 32 -- the last chunk of 32 dimensions is ragged
CHUNKS = {"nearest_chunk": 256, "separation_chunk": 256, "trust_chunk": 256}  # every family runs several chunks


def flat(result, name="result"):
    """-> [(path, value)] of a call's result: tuples and named tuples unfolded, every `seconds` field left out."""
    if isinstance(result, tuple):
        names = getattr(result, "_fields", range(len(result)))
        return [leaf for field, v in zip(names, result) if field != "seconds" for leaf in flat(v, "%s.%s" % (name, field))]
    return [(name, result)]


def calls(size):
    """-> [(name, call(engine))]: one call of every family at `size` ("small" | "large"), and the three that are the same in every round."""
    rng = np.random.default_rng(7)
    big = size == "large"
    lab = rng.integers(0, 7, N).astype(np.int64)
    Y = np.ascontiguousarray(rng.standard_normal((N, 2)).astype(np.float32))
    nq, nk = (600, 17) if big else (10, 3)
    q = rng.permutation(N)[:nq].astype(np.uint32)
    m, classes = (3000, 5) if big else (50, 2)  # 3000 samples: three sample blocks of 1024
    ids = rng.integers(0, N, m).astype(np.uint32)
    y = (rng.random((m, classes)) < 0.4).astype(np.uint8)
    W = 0.1 * rng.standard_normal((classes, D + 1))
    sil = None if big else rng.permutation(N)[:20].astype(np.uint32)
    tq, tk = (None, 12) if big else (rng.permutation(N)[:30].astype(np.uint32), 3)

    def fit_and_decide(e):
        model = e.logreg_fit(ids=ids, y=y, max_iter=4)
        return model, e.logreg_decision(model, ids=ids)

    return [("nearest", lambda e: e.nearest(ids=q, k=nk, metric="cos")),
            ("kmeans", lambda e: e.kmeans(40 if big else 3, max_iters=8, seed=1)),
            ("logreg_eval", lambda e: e.logreg_eval(W, y, ids=ids)),
            ("davies_bouldin", lambda e: e.davies_bouldin(lab, details=True)),
            ("silhouette", lambda e: e.silhouette(lab, ids=sil, samples=True)),
            ("logreg_fit", fit_and_decide),
            ("modularity", lambda e: e.modularity(lab)),
            ("trustworthiness", lambda e: e.trustworthiness(Y, tk, tq, samples=True)),
            ("pca", lambda e: e.pca(2, details=True)),
            ("recall", lambda e: e.neighbour_recall(k=nk, metric="l2", ids=q))]


def engine():
    eng = engine_for((np.random.default_rng(3).standard_normal((N, D)) + np.repeat(np.arange(N) % 5, D).reshape(N, D)).astype(np.float32))
    for name, value in CHUNKS.items():
        eng.set_param(name, value)
    return eng


@gpu
def test_interleaved_calls_on_one_handle_equal_fresh_handles_bit_for_bit():
    want = {}
    for size in ("small", "large"):
        for name, call in calls(size):
            eng = engine()
            try:
                want[size, name] = flat(call(eng))
            finally:
                eng.close()
    eng = engine()
    try:
        for size in ("small", "large", "small"):
            for name, call in calls(size):
                got = flat(call(eng))
                assert [p for p, _ in got] == [p for p, _ in want[size, name]]
                for (path, a), (_, b) in zip(got, want[size, name]):
                    assert np.array_equal(np.asarray(a), np.asarray(b)), (size, name, path)
    finally:
        eng.close()
    large = dict(want["large", "trustworthiness"])
    assert len(large["result.samples_x"]) == N and len(dict(want["large", "silhouette"])["result.1"]) == N  # the large round took every vertex
