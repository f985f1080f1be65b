// f2v_layout.hip.h -- a principal-component layout of the embedding matrix and how faithful a layout is: f2v_pca and
// f2v_trustworthiness (include/f2v.h, "layout").
//
// PCA.  The mean and the scatter matrix are fp64 sums over the vertices in pieces of 4096 consecutive vertices:
//   pca_colsum_kernel     one thread per (piece, dimension): the piece's column sum, sequentially;
//   pca_reduce_kernel     one thread per entry: the piece results added in piece order, divided (by n for the mean, by 1 for the scatter);
//   pca_scatter_kernel    one workgroup = one piece x one 64 x 64 tile of (d, e) entries, only tiles that hold an entry d <= e.  The
//                         piece's rows pass through LDS 32 at a time (16-byte loads, the next batch in flight while this one is
//                         multiplied), already centred: z = (double)x - mean once per staged element.  A thread owns a 4 x 4 register
//                         tile of fp64 accumulators and walks the batch's vertices in order, so an entry's chain is the definition's
//                         fma(z_vd, z_ve, acc) over ascending vertex id.  A row slot past the piece's end reads the piece's last row
//                         and is never walked, a dimension past D is a zero whose entries are never stored;
//   pca_project_kernel    one thread per (vertex, component): the fp64 fma chain over ascending d, rounded to fp32.
// The D x D eigenproblem is the host's (pca_jacobi_host, f2v_host.cpp).
//
// Trustworthiness.  The k nearest rows in both spaces come from nearest_kernel as it is.  Then, per space M and chunk of samples,
//   trust_keys_kernel     one workgroup per sample: the threshold key (distance to the target by the fp32 chain, target id) of each
//                         of its up to k targets -- a target that is among the sample's own k nearest in M cannot have a place above
//                         k and gets the pad key -- sorted descending (pads first) by counting;
//   trust_rank_kernel     the hot path, separation_pair_kernel's tiling (sample block x candidate span, chunks of 32 dimensions
//                         through LDS, a lane owns two sample rows and eight candidates, packed fp32 subtract and fma, accumulators
//                         persisting over the chunks) with a compare-and-count epilogue: a candidate's key is compared with the
//                         sample's farthest threshold first -- most candidates end there -- and otherwise binary-searched into the
//                         sample's sorted thresholds; the slot it lands in is counted in an LDS histogram (integer atomics), the
//                         workgroup's histograms are added to the chunk's in HBM (integer atomics);
//   trust_finish_kernel   one thread per sample: the histogram's prefix sums are the numbers of candidates before each target,
//                         place - k where positive is added up.
// Integer counts only: what a sample's penalty is cannot depend on spans, blocks or the order in which workgroups run.
#ifndef F2V_LAYOUT_HIP_H_
#define F2V_LAYOUT_HIP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f2v_nearest.hip.h"
#include "f2v_separation.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kPcaPiece = 4096;  // F2V_PCA_PIECE
constexpr uint32_t kPcaTile = 64;     // (d, e) entries per side of a workgroup's tile
constexpr uint32_t kPcaBatch = 32;    // rows staged per step
constexpr uint32_t kPcaThreads = 256;
constexpr uint32_t kTrustMaxSpan = 4096;  // most candidates per workgroup of trust_rank_kernel
constexpr nn_key_t kTrustPad = ~0ull;     // the key of a target that is not ranked: no candidate's key is greater

// part[piece][d] = x[lo][d] + x[lo + 1][d] + ... in fp64, sequentially from +0.  grid (pieces, ceil(D / 64))
__global__ __launch_bounds__(64) void pca_colsum_kernel(const float *X, uint32_t n, uint32_t D, double *part) {
    const uint32_t d = blockIdx.y * blockDim.x + threadIdx.x, piece = blockIdx.x;
    if (d >= D) return;
    const uint32_t lo = piece * kPcaPiece, hi = n - lo < kPcaPiece ? n : lo + kPcaPiece;
    double s = 0.0;
    for (uint32_t v = lo; v < hi; v++) s += (double)X[(size_t)v * D + d];
    part[(size_t)piece * D + d] = s;
}

// out[i] = (part[0][i] + part[1][i] + ... sequentially from +0) / denom
__global__ void pca_reduce_kernel(const double *part, uint32_t pieces, size_t width, double denom, double *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width) return;
    double s = 0.0;
    for (uint32_t p = 0; p < pieces; p++) s += part[(size_t)p * width + i];
    out[i] = s / denom;
}

struct PcaScatterArgs {
    const float *X;      // n x D, the settled matrix
    const double *mean;  // D
    double *ws;          // [piece][packed (d, e), d <= e]: the piece's chains
    size_t width;        // D (D + 1) / 2
    uint32_t n, D, tiles;  // tiles = ceil(D / 64) per side
};

// the place of entry (d, e), d <= e, in a packed upper triangle
__host__ __device__ inline size_t pca_packed(uint32_t D, uint32_t d, uint32_t e) { return (size_t)d * D - (size_t)d * (d + 1) / 2 + e; }

// grid (pieces, tiles (tiles + 1) / 2), 256 threads = 16 x 16: thread (tx, ty) owns d = 64 td + 4 tx + i, e = 64 te + 4 ty + j.
// Staging: thread t loads the 16-byte piece t & 31 of a row's 128 staged floats (64 of the d tile, 64 of the e tile) for rows
// t >> 5, (t >> 5) + 8 ... of the batch: its four dimensions, hence its four means, are the same for every row.
__global__ __launch_bounds__(256) void pca_scatter_kernel(const PcaScatterArgs a) {
    __shared__ __attribute__((aligned(16))) double Zs[kPcaBatch * 2 * kPcaTile];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4, piece = blockIdx.x;
    uint32_t td = 0, te = blockIdx.y;
    while (te >= a.tiles - td) {
        te -= a.tiles - td;
        td++;
    }
    te += td;
    const uint32_t lo = piece * kPcaPiece, cnt = a.n - lo < kPcaPiece ? a.n - lo : kPcaPiece;
    const uint32_t c = tid & 31u, r0 = tid >> 5;
    const uint32_t dim0 = c < 16 ? td * kPcaTile + 4 * c : te * kPcaTile + 4 * (c - 16);
    double m[4];
#pragma unroll
    for (int q = 0; q < 4; q++) m[q] = a.mean[dim0 + q < a.D ? dim0 + q : 0];
#pragma unroll
    for (int q = 0; q < 4; q++) m[q] = dim0 + q < a.D ? m[q] : 0.0;
    float4 pre[4];
    auto load = [&](uint32_t b) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t r = b * kPcaBatch + r0 + 8 * i;
            pre[i] = sep_load4(a.X, a.D, lo + (r < cnt ? r : cnt - 1), dim0);
        }
    };
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    auto step = [&](uint32_t v) {
        const double *z = Zs + v * 2 * kPcaTile;
        double za[4], zb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            za[i] = z[4 * tx + i];
            zb[i] = z[kPcaTile + 4 * ty + i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = __builtin_fma(za[i], zb[j], acc[i][j]);
    };
    const uint32_t nb = (cnt + kPcaBatch - 1) / kPcaBatch;
    load(0);
    for (uint32_t b = 0; b < nb; b++) {
        __syncthreads();  // the previous batch has been walked
#pragma unroll
        for (int i = 0; i < 4; i++) {
            double *o = Zs + (r0 + 8 * i) * 2 * kPcaTile + 4 * c;
            o[0] = (double)pre[i].x - m[0];
            o[1] = (double)pre[i].y - m[1];
            o[2] = (double)pre[i].z - m[2];
            o[3] = (double)pre[i].w - m[3];
        }
        __syncthreads();
        if (b + 1 < nb) load(b + 1);  // the next batch travels while this one is multiplied
        const uint32_t left = cnt - b * kPcaBatch;
        if (left >= kPcaBatch) {
#pragma unroll 4
            for (uint32_t v = 0; v < kPcaBatch; v++) step(v);
        } else {
            for (uint32_t v = 0; v < left; v++) step(v);  // the piece's rows only: a stand-in is never walked
        }
    }
    double *out = a.ws + (size_t)piece * a.width;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t d = td * kPcaTile + 4 * tx + i, e = te * kPcaTile + 4 * ty + j;
            if (d <= e && e < a.D) out[pca_packed(a.D, d, e)] = acc[i][j];
        }
}

// Y[v][c] = (float) chain_d fma((double)x_vd - mean_d, W[c][d], acc) from +0 over ascending d
__global__ void pca_project_kernel(const float *X, const double *mean, const double *W, uint32_t n, uint32_t D, uint32_t d2, float *Y) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * d2) return;
    const float *x = X + idx / d2 * D;
    const double *w = W + idx % d2 * D;
    double acc = 0.0;
    for (uint32_t d = 0; d < D; d++) acc = __builtin_fma((double)x[d] - mean[d], w[d], acc);
    Y[idx] = (float)acc;
}

// ---- trustworthiness ---------------------------------------------------------------------------------------------------------------
struct TrustKeyArgs {
    const float *M;             // rows x D: the space the targets are ranked in
    const uint32_t *sid;        // this launch's samples (vertex ids)
    const uint32_t *tgt;        // [sample][k]: the targets (the sample's k nearest in the OTHER space)
    const uint32_t *own;        // [sample][k]: the sample's k nearest in M
    nn_key_t *thr;              // [sample][k]: the targets' keys, descending, pads first
    unsigned long long *hits;   // += targets that are among `own` (nullptr: not counted)
    uint32_t n, D, k;
};

// grid samples, 128 threads: thread t = target slot t.  (2 k < n: the lists of k nearest are full, every target is a vertex; a slot
// that held none would be a pad.)
__global__ __launch_bounds__(128) void trust_keys_kernel(const TrustKeyArgs a) {
    __shared__ nn_key_t ks[kNnMaxK];
    __shared__ uint32_t ow[kNnMaxK];
    __shared__ uint32_t shared_cnt;
    const uint32_t q = blockIdx.x, t = threadIdx.x, i = a.sid[q];
    if (t == 0) shared_cnt = 0;
    if (t < a.k) ow[t] = a.own[(size_t)q * a.k + t];
    __syncthreads();
    nn_key_t key = kTrustPad;
    if (t < a.k) {
        const uint32_t j = a.tgt[(size_t)q * a.k + t];
        bool both = false;
        for (uint32_t u = 0; u < a.k; u++) both |= ow[u] == j;
        if (both) {
            atomicAdd(&shared_cnt, 1u);
        } else if (j < a.n) {
            const float *x = a.M + (size_t)i * a.D, *y = a.M + (size_t)j * a.D;
            float acc = 0.f;
            for (uint32_t d = 0; d < a.D; d++) {
                const float s = x[d] - y[d];
                acc = __builtin_fmaf(s, s, acc);
            }
            key = nn_make_key(-acc, j);
        }
        ks[t] = key;
    }
    __syncthreads();
    if (t < a.k) {
        uint32_t place = 0;  // keys greater than this one; equal keys are pads: by slot
        for (uint32_t u = 0; u < a.k; u++) place += (ks[u] > key || (ks[u] == key && u < t)) ? 1u : 0u;
        a.thr[(size_t)q * a.k + place] = key;
    }
    if (t == 0 && a.hits && shared_cnt) atomicAdd(a.hits, (unsigned long long)shared_cnt);
}

struct TrustRankArgs {
    const float *M;        // rows x D
    const uint32_t *sid;   // this launch's samples (vertex ids)
    const nn_key_t *thr;   // [sample][k] sorted descending, pads first
    uint32_t *hist;        // [sample][k]: += candidates whose first threshold below them is that slot
    uint32_t n, D, nq, k, blocks, span;  // span: candidates per workgroup (a multiple of 64)
};

__host__ __device__ inline size_t trust_lds_bytes(uint32_t rb, uint32_t k) {
    const size_t sw = (size_t)(kSepThreads / (rb / 2)) * kSepAcc;
    return ((size_t)(rb / 2) * kSepXStride + sw * kSepCStride) * sizeof(float) + (size_t)rb * k * (sizeof(nn_key_t) + sizeof(uint32_t));
}

// the slot of the first threshold that `key` is greater than (the caller knows it is greater than the last one)
__device__ inline void trust_count(const nn_key_t *t, uint32_t *h, uint32_t k, nn_key_t key) {
    uint32_t lo = 0, hi = k - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key > t[mid]) hi = mid;
        else lo = mid + 1;
    }
    atomicAdd(h + lo, 1u);
}

// grid spans x blocks (the sample blocks of one span are neighbours: they share the span's rows in L2), 256 threads laid out as in
// separation_pair_kernel.  A sample row past the launch's last reads the last sample and counts nothing (its thresholds are pads), a
// candidate past the span's end reads the span's last row and is not counted.
template <int RB>
__global__ __launch_bounds__(256) void trust_rank_kernel(const TrustRankArgs a) {
    constexpr uint32_t HP = RB / 2, G = kSepThreads / HP, SW = G * kSepAcc;
    constexpr int XP = RB / 64;
    constexpr int CP = SW / 32;
    extern __shared__ float4 trust_smem[];
    float *Xs = reinterpret_cast<float *>(trust_smem);               // [pair][d][2]: one chunk of the sample block
    float *Cs = Xs + HP * kSepXStride;                               // [candidate][d]: one chunk of the sweep's candidates
    nn_key_t *thr = reinterpret_cast<nn_key_t *>(Cs + SW * kSepCStride);  // [sample row][k]
    uint32_t *hist = reinterpret_cast<uint32_t *>(thr + (size_t)RB * a.k);

    const uint32_t tid = threadIdx.x, rp = tid % HP, g = tid / HP;
    const uint32_t span = blockIdx.x / a.blocks, row0 = (blockIdx.x % a.blocks) * RB;
    const uint32_t m0 = span * a.span, cnt = a.n - m0 < a.span ? a.n - m0 : a.span;
    const uint32_t nch = (a.D + kSepChunk - 1) / kSepChunk, nsw = (cnt + SW - 1) / SW;
    const uint32_t q4 = 4 * (tid & 7u);

    for (uint32_t i = tid; i < (uint32_t)RB * a.k; i += kSepThreads) {
        const uint32_t r = row0 + i / a.k;
        thr[i] = r < a.nq ? a.thr[(size_t)r * a.k + i % a.k] : kTrustPad;
        hist[i] = 0;
    }
    const uint32_t my0 = a.sid[row0 + rp < a.nq ? row0 + rp : a.nq - 1], my1 = a.sid[row0 + rp + HP < a.nq ? row0 + rp + HP : a.nq - 1];

    uint32_t xv0[XP], xv1[XP];
    sep_samples<XP>(a.sid, row0, a.nq, HP, tid, xv0, xv1);
    float4 px0[XP], px1[XP], pc[CP];
    auto load = [&](uint32_t sweep, uint32_t d0) {
#pragma unroll
        for (int i = 0; i < XP; i++) {
            px0[i] = sep_load4(a.M, a.D, xv0[i], d0 + q4);
            px1[i] = sep_load4(a.M, a.D, xv1[i], d0 + q4);
        }
#pragma unroll
        for (int i = 0; i < CP; i++) {
            const uint32_t m = sweep * SW + ((tid + kSepThreads * i) >> 3);
            pc[i] = sep_load4(a.M, a.D, m0 + (m < cnt ? m : cnt - 1), d0 + q4);
        }
    };
    load(0, 0);

    for (uint32_t s = 0; s < nsw; s++) {
        sep_f2 acc[kSepAcc];
#pragma unroll
        for (int e = 0; e < (int)kSepAcc; e++) acc[e] = sep_f2{0.f, 0.f};
        for (uint32_t c = 0; c < nch; c++) {
            __syncthreads();  // the previous chunk has been read (and, the first time, the thresholds are in place)
            sep_stage<XP, CP>(Xs, Cs, px0, px1, pc, tid, q4);
            __syncthreads();
            // the next chunk (or the next sweep's first) travels while this one is scored
            if (c + 1 < nch) load(s, (c + 1) * kSepChunk);
            else if (s + 1 < nsw) load(s + 1, 0);
            sep_score<G>(Xs, Cs, rp, g, acc);
        }
        // compare and count: the farthest threshold first (most candidates are farther than every target and end here)
        const nn_key_t lim0 = thr[(size_t)rp * a.k + a.k - 1], lim1 = thr[(size_t)(rp + HP) * a.k + a.k - 1];
#pragma unroll
        for (int e = 0; e < (int)kSepAcc; e++) {
            const uint32_t m = s * SW + g + G * e, cand = m0 + m;
            if (m >= cnt) continue;  // a stand-in: scored, never counted
            const nn_key_t k0 = nn_make_key(-acc[e].x, cand), k1 = nn_make_key(-acc[e].y, cand);
            if (k0 > lim0 && cand != my0) trust_count(thr + (size_t)rp * a.k, hist + (size_t)rp * a.k, a.k, k0);
            if (k1 > lim1 && cand != my1) trust_count(thr + (size_t)(rp + HP) * a.k, hist + (size_t)(rp + HP) * a.k, a.k, k1);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)RB * a.k; i += kSepThreads) {
        const uint32_t r = row0 + i / a.k, h = hist[i];
        if (h && r < a.nq) atomicAdd(a.hist + (size_t)r * a.k + i % a.k, h);
    }
}

// penalty[q] = sum over the ranked targets of max(0, place - k), place = 1 + the candidates before the target = 1 + the prefix sum of
// the histogram up to the target's slot; *sum += penalty[q].  One thread per sample.
__global__ void trust_finish_kernel(const nn_key_t *thr, const uint32_t *hist, uint32_t nq, uint32_t k, unsigned long long *penalty,
                                    unsigned long long *sum) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    unsigned long long before = 0, pen = 0;
    for (uint32_t s = 0; s < k; s++) {
        before += hist[(size_t)q * k + s];
        if (thr[(size_t)q * k + s] != kTrustPad && before + 1 > k) pen += before + 1 - k;
    }
    penalty[q] = pen;
    if (pen) atomicAdd(sum, pen);
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_LAYOUT_HIP_H_
