// f2v_logreg.hip.h -- one-vs-rest logistic regression on rows of the embedding matrix or on per-pair features of two rows
// (include/f2v.h, "logistic regression").
//
//   logreg_kernel<true, NA, NZ>   one workgroup per (block of 1024 consecutive samples, group of classes).  The group's weights are
//                          resident in LDS as doubles.  The block passes in tiles of 32 samples: the rows are gathered with 16-byte
//                          loads, the pair feature is formed in registers and the tile is staged in LDS as floats; a thread then owns
//                          one sample and NZ classes (lane groups of 32 share out the classes round robin) and runs their fp64 fma
//                          chains over ascending d, reading a feature once for all its classes, and leaves r and the loss term in
//                          LDS; the gradient sums live in registers, NA to a thread, lanes over (class, dimension), and take the
//                          tile's samples one after the other, which is the order f2v.h defines; the bias gradients and the losses
//                          are one more sum of the first threads.  One partial per block goes to the workspace.
//   logreg_kernel<false, 1, NZ>      the logits phase alone: z of every (sample, class) for f2v_logreg_decision.
//   logreg_reduce_kernel   adds the block partials in ascending block order.
// Everything is VALU fp64; no float atomics, no atomics at all: every result is a function of its inputs alone.
#ifndef F2V_LOGREG_HIP_H_
#define F2V_LOGREG_HIP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kLrThreads = 256;
constexpr uint32_t kLrBlock = 1024;      // F2V_LOGREG_BLOCK
constexpr uint32_t kLrMaxClasses = 64;   // F2V_LOGREG_MAX_CLASSES
constexpr uint32_t kLrTile = 32;         // samples staged at a time
constexpr uint32_t kLrGroups = kLrThreads / kLrTile;      // lane groups of the logits phase: group g takes classes g, g + 8, ...
constexpr uint32_t kLrAcc = 32;          // gradient sums a thread carries at most: 64 classes x 128 dimensions over 256 threads
constexpr uint32_t kLrLdsBytes = 144 * 1024;  // what a workgroup may ask for

enum { kLrRow = -1, kLrHadamard = 0, kLrL1 = 1, kLrL2 = 2, kLrAverage = 3 };  // F2V_PAIR_*; kLrRow: no second id

struct LrArgs {
    const float *X;        // n x D, the settled matrix
    const uint32_t *a, *b; // m sample ids (b: pairs only)
    const uint8_t *y;      // m x C targets (eval)
    const uint32_t *cmap;  // nc: the target column of every evaluated class (eval)
    const double *W;       // nc x (D + 1), bias last
    double *out;           // eval: [blocks][nc][D + 2] partials (gradient of the D weights, of the bias, the loss); decision: [m][nc]
    uint32_t m, D, nc, C, cg, lg;  // nc: classes evaluated, C: columns of y, cg: classes per workgroup, lg: lr_log2(D)
    int feature;
};

__host__ __device__ inline uint32_t lr_stride(uint32_t D) { return D | 1u; }  // floats per staged sample: odd, so that lanes over samples meet no bank twice

__host__ __device__ inline size_t lr_lds_bytes(uint32_t D, uint32_t cg) {
    return sizeof(double) * ((size_t)cg * (D + 1) + (size_t)kLrTile * 2 * cg) + sizeof(float) * (size_t)kLrTile * lr_stride(D);
}

__host__ __device__ inline uint32_t lr_log2(uint32_t D) {  // the power of two that holds D (D <= 512)
    uint32_t lg = 0;
    while ((1u << lg) < D) lg++;
    return lg;
}

// classes per workgroup: as many of `nc` as the accumulators and the LDS hold (16 at least for every D <= 512)
__host__ __device__ inline uint32_t lr_group(uint32_t D, uint32_t nc) {
    uint32_t cg = (kLrThreads * kLrAcc) >> lr_log2(D);
    if (cg > kLrMaxClasses) cg = kLrMaxClasses;
    while (cg > 1 && lr_lds_bytes(D, cg) > kLrLdsBytes) cg--;
    return cg < nc ? cg : nc;
}

// the feature of f2v.h, one rounding per operation; every form is computed and one is kept, so that no branch enters the gather loop
__device__ inline float lr_feature(int feature, float xa, float xb) {
    const float t = xa - xb;
    const float v = feature == kLrHadamard ? xa * xb : feature == kLrL1 ? __builtin_fabsf(t) : feature == kLrL2 ? t * t : (xa + xb) * 0.5f;
    return feature == kLrRow ? xa : v;
}

// -> (r, loss term) of one (sample, class): sigma(z) - y and softplus(z) - y z as f2v.h defines them.
__device__ inline double2 lr_terms(double z, double y) {
    const double en = exp(-__builtin_fabs(z));  // in (0, 1]: exp(-z) for z >= 0, exp(z) below
    const double sp = __builtin_fmax(z, 0.0) + log1p(en);
    const double sg = z >= 0.0 ? 1.0 / (1.0 + en) : en / (1.0 + en);
    return make_double2(sg - y, sp - y * z);
}

// grid (ceil(m / 1024), ceil(nc / cg)), 256 threads
template <bool EVAL, int NA, int NZ>
__global__ __launch_bounds__(256) void logreg_kernel(const LrArgs p) {
    extern __shared__ double lr_smem[];
    const uint32_t D = p.D, cg = p.cg, stride = lr_stride(D), E = D + 2;
    double *Ws = lr_smem;                                   // [cg][D + 1]
    double *R2 = Ws + (size_t)cg * (D + 1);                 // [tile][2 cg]: r of every class, then the loss terms
    float *Fs = reinterpret_cast<float *>(R2 + (size_t)kLrTile * 2 * cg);  // [tile][stride]: the features

    const uint32_t tid = threadIdx.x;
    const uint32_t c0 = blockIdx.y * cg, gc = p.nc - c0 < cg ? p.nc - c0 : cg;
    const uint32_t base = blockIdx.x * kLrBlock, bcnt = p.m - base < kLrBlock ? p.m - base : kLrBlock;
    for (uint32_t i = tid; i < gc * (D + 1); i += kLrThreads) Ws[i] = p.W[(size_t)c0 * (D + 1) + i];

    // logits: sample s of the tile, classes g, g + 8, ... of the group (a slot past the group repeats its last class and is dropped)
    const uint32_t s = tid % kLrTile, g = tid / kLrTile;
    uint32_t woff[NZ];
#pragma unroll
    for (int k = 0; k < NZ; k++) {
        const uint32_t c = g + kLrGroups * k;
        woff[k] = (c < gc ? c : gc - 1) * (D + 1);
    }
    // gradient: slot q = tid + 256 j of the group's classes x Dp dimensions, Dp = 1 << lg the power of two that holds D: class q >> lg,
    // dimension q & (Dp - 1), which depends on j's parity alone as Dp <= 512 (a slot past D or past the group repeats the last
    // dimension or class and is dropped).  The bias gradients and the losses, two entries per class, are one more accumulator of the first 2 gc threads.
    const uint32_t lg = p.lg, d0 = tid & ((1u << lg) - 1u), d1 = (tid + kLrThreads) & ((1u << lg) - 1u);
    const uint32_t fo0 = __builtin_elementwise_min(d0, D - 1), fo1 = __builtin_elementwise_min(d1, D - 1);
    const uint32_t bo = tid < 2 * gc ? (tid & 1u) * cg + (tid >> 1) : 0;
    double acc[NA], acc2 = 0.0;
    uint32_t ro[NA];
    if (EVAL) {
#pragma unroll
        for (int j = 0; j < NA; j++) {
            const uint32_t c = (tid + kLrThreads * j) >> lg;
            acc[j] = 0.0;
            ro[j] = __builtin_elementwise_min(c, gc - 1);  // (a minimum, not a select: no lane mask is kept per sum)
        }
    }

    for (uint32_t t0 = 0; t0 < bcnt; t0 += kLrTile) {
        const uint32_t cnt = bcnt - t0 < kLrTile ? bcnt - t0 : kLrTile;
        __syncthreads();  // the previous tile has been read (first tile: nothing yet)
        if ((D & 3u) == 0) {
            const uint32_t nq = D >> 2;
            for (uint32_t idx = tid; idx < cnt * nq; idx += kLrThreads) {
                const uint32_t ss = idx / nq, q = idx % nq;
                const size_t i = (size_t)base + t0 + ss;
                float4 v = *reinterpret_cast<const float4 *>(p.X + (size_t)p.a[i] * D + 4 * q);
                if (p.feature != kLrRow) {
                    const float4 u = *reinterpret_cast<const float4 *>(p.X + (size_t)p.b[i] * D + 4 * q);
                    v = make_float4(lr_feature(p.feature, v.x, u.x), lr_feature(p.feature, v.y, u.y), lr_feature(p.feature, v.z, u.z),
                                    lr_feature(p.feature, v.w, u.w));
                }
                float *o = Fs + ss * stride + 4 * q;
                o[0] = v.x;
                o[1] = v.y;
                o[2] = v.z;
                o[3] = v.w;
            }
        } else {
            for (uint32_t idx = tid; idx < cnt * D; idx += kLrThreads) {
                const uint32_t ss = idx / D, d = idx % D;
                const size_t i = (size_t)base + t0 + ss;
                float v = p.X[(size_t)p.a[i] * D + d];
                if (p.feature != kLrRow) v = lr_feature(p.feature, v, p.X[(size_t)p.b[i] * D + d]);
                Fs[ss * stride + d] = v;
            }
        }
        __syncthreads();  // (also: the weights are in place)

        if (s < cnt) {
            double z[NZ];
#pragma unroll
            for (int k = 0; k < NZ; k++) z[k] = 0.0;
            const float *fs = Fs + s * stride;
            for (uint32_t d = 0; d < D; d++) {
                const double f = (double)fs[d];
#pragma unroll
                for (int k = 0; k < NZ; k++)
                    z[k] = __builtin_fma(f, Ws[woff[k] + d], z[k]);
            }
            const size_t i = (size_t)base + t0 + s;
#pragma unroll
            for (int k = 0; k < NZ; k++) {
                const uint32_t c = g + kLrGroups * k;
                if (c < gc) {
                    const double zz = z[k] + Ws[c * (D + 1) + D];
                    if (EVAL) R2[s * 2 * cg + c] = zz;  // the thread's own slot: read back below
                    else p.out[i * p.nc + c0 + c] = zz;
                }
            }
            if (EVAL) {
#pragma unroll 1
                for (uint32_t c = g; c < gc; c += kLrGroups) {  // rolled: one copy of exp and log1p in the kernel
                    double *slot = R2 + s * 2 * cg + c;
                    const double zz = *slot;
                    const double yv = (double)p.y[i * p.C + p.cmap[c0 + c]];
                    const double2 t = lr_terms(zz, yv);
                    slot[0] = t.x;
                    slot[cg] = t.y;
                }
            }
        }
        if (EVAL) {
            __syncthreads();
#pragma unroll 2
            for (uint32_t ss = 0; ss < cnt; ss++) {
                const double *r = R2 + ss * 2 * cg;
                const double f0 = (double)Fs[ss * stride + fo0], f1 = (double)Fs[ss * stride + fo1];
#pragma unroll
                for (int j = 0; j < NA; j++) acc[j] = __builtin_fma(r[ro[j]], (j & 1) ? f1 : f0, acc[j]);
                acc2 += r[bo];
            }
        }
    }
    if (EVAL) {
        double *o = p.out + ((size_t)blockIdx.x * p.nc + c0) * E;
#pragma unroll
        for (int j = 0; j < NA; j++) {
            const uint32_t q = tid + kLrThreads * j, c = q >> lg, d = q & ((1u << lg) - 1u);
            if (c < gc && d < D) o[c * E + d] = acc[j];
        }
        if (tid < 2 * gc) o[(tid >> 1) * E + D + (tid & 1u)] = acc2;
    }
}

// out[e] = part[0][e] + part[1][e] + ... sequentially from +0, e < entries (= nc x (D + 2))
__global__ __launch_bounds__(256) void logreg_reduce_kernel(const double *part, uint32_t blocks, uint32_t entries, double *out) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= entries) return;
    double sum = 0.0;
    for (uint32_t b = 0; b < blocks; b++) sum += part[(size_t)b * entries + e];
    out[e] = sum;
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_LOGREG_HIP_H_
