// f2v_kmeans.hip.h -- k-means clustering of the embedding matrix and the modularity of a labelling (include/f2v.h, "clustering";
// DESIGN section 10).
//
// One Lloyd iteration is
//   kmeans_assign_kernel    rows stream through once in blocks of RB (coalesced 16-byte loads, staged through LDS in chunks of 32
//                           dimensions as nearest_kernel stages its candidates), the centroids are the resident side (LDS: all of
//                           them where K x D fits kKmTileFloats, tiles otherwise); a thread owns TWO ROWS and up to kKmAcc centroids
//                           per sweep -- lane = row pair, so a wave is busy whatever K is, and the centroids of a sweep are dealt
//                           round robin to the workgroup's 512 / RB lane groups, so K = 8 occupies all eight groups of RB = 64;
//                           distance = the fp32 chain of f2v.h, selection = the nearest-neighbour key order with k = 1;
//   kmeans_hist / offsets / starts / scatter_kernel   a stable counting sort of the vertices by label: the members of every cluster
//                           in ascending id, whatever order workgroups run in (integer LDS atomics only);
//   kmeans_piece_sum_kernel one piece of 64 members per lane group, lanes over dimensions, eight member rows in flight, fp64;
//   kmeans_centroid_kernel  a cluster's piece sums added in piece order (fp64), divided, rounded; an empty cluster is left alone.
// kmeans_inertia_piece / _reduce_kernel sum the fp32 distances in the fixed order of f2v.h; modularity_kernel tallies the simple
// graph's edges by community with integer atomics.  No float atomics anywhere: every result is a function of its inputs alone.
#ifndef F2V_KMEANS_HIP_H_
#define F2V_KMEANS_HIP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f2v_nearest.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kKmThreads = 256;
constexpr uint32_t kKmAcc = 8;              // centroids a thread scores per sweep (for each of its two rows)
constexpr uint32_t kKmPiece = 64;           // F2V_KMEANS_PIECE
constexpr uint32_t kKmMaxK = 1024;          // F2V_KMEANS_MAX_K
constexpr uint32_t kKmSortBlock = 1024;     // vertices per workgroup of the counting sort
constexpr uint32_t kKmTileFloats = 16384;   // centroid values resident in LDS at a time (64 KiB), one sweep's worth at least
constexpr uint32_t kKmSumTile = 64;         // piece sums kmeans_centroid_kernel stages per step
constexpr uint32_t kModLdsClusters = 2048;  // modularity_kernel tallies in LDS up to this many communities

struct KmAssignArgs {
    const float *X;     // n x D, the settled matrix
    const float *C;     // k x D centroids
    uint32_t *labels;   // n: read (the previous labels) and written
    float *dist;        // n: distance to the chosen centroid
    uint32_t *changed;  // += rows whose label changed
    uint32_t n, D, k, tile;  // tile: centroids resident at a time (a multiple of the sweep width, or k)
};

__host__ __device__ constexpr uint32_t km_sweep(uint32_t rb) { return (2 * kKmThreads / rb) * kKmAcc; }

// centroids resident at a time: all of them where they fit kKmTileFloats, else as many whole sweeps as fit (one at least)
__host__ __device__ inline uint32_t km_tile(uint32_t rb, uint32_t D, uint32_t k) {
    const uint32_t Dp = (D + kNnChunk - 1) / kNnChunk * kNnChunk, sw = km_sweep(rb);
    if ((size_t)k * Dp <= kKmTileFloats) return k;
    const uint32_t sweeps = kKmTileFloats / Dp / sw;
    const uint32_t t = (sweeps ? sweeps : 1u) * sw;
    return t < k ? t : k;
}

__host__ __device__ inline size_t km_lds_bytes(uint32_t rb, uint32_t D, uint32_t tile) {
    const size_t Dp = (D + kNnChunk - 1) / kNnChunk * kNnChunk;
    return ((size_t)tile * Dp + (size_t)rb * kNnStride) * sizeof(float) + (size_t)(2 * kKmThreads / rb) * rb * sizeof(nn_key_t) + 16;
}

// The workgroup's loads of one chunk of its row block: thread t takes 16-byte piece t, t + 256 ... (eight pieces to a row's chunk).
// A row past the matrix reads the last row instead (its result is never stored), dimensions past D become zeros: the only condition
// is the chunk's own, nothing is kept across the loads.
template <int PRE>
__device__ inline void km_load_rows(float4 (&pre)[PRE], const float *X, uint32_t n, uint32_t D, uint32_t row0, uint32_t d0, uint32_t tid) {
    const uint32_t d = d0 + 4 * (tid & 7u);
    if ((D & 3u) == 0) {
        const uint32_t dd = d < D ? d : 0;
#pragma unroll
        for (int i = 0; i < PRE; i++) {
            const uint32_t row = row0 + ((tid + kKmThreads * i) >> 3);
            const float4 v = *reinterpret_cast<const float4 *>(X + (size_t)(row < n ? row : n - 1) * D + dd);
            pre[i] = d < D ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
#pragma unroll
        for (int i = 0; i < PRE; i++) {
            const uint32_t row = row0 + ((tid + kKmThreads * i) >> 3);
            const float *p = X + (size_t)(row < n ? row : n - 1) * D;
            float e[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float v = p[d + q < D ? d + q : 0];
                e[q] = d + q < D ? v : 0.f;
            }
            pre[i] = make_float4(e[0], e[1], e[2], e[3]);
        }
    }
}

// grid ceil(n / RB), 256 threads = 512 / RB lane groups of RB / 2 lanes; lane = rows (rp, rp + RB / 2) of the block, group g scores
// centroids g, g + G, g + 2G ... of a sweep
template <int RB>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const KmAssignArgs a) {
    constexpr uint32_t HP = RB / 2, G = kKmThreads / HP, SW = G * kKmAcc;
    constexpr int PRE = RB / 32;  // 16-byte loads per thread and chunk
    extern __shared__ float4 km_smem[];
    const uint32_t nch = (a.D + kNnChunk - 1) / kNnChunk, Dp = nch * kNnChunk;
    float *Cs = reinterpret_cast<float *>(km_smem);  // [tile][Dp], zeros behind dimension D
    float *Xs = Cs + (size_t)a.tile * Dp;            // [RB][kNnStride]: one chunk of the row block
    nn_key_t *best = reinterpret_cast<nn_key_t *>(Xs + RB * kNnStride);  // [G][RB]
    uint32_t *nchanged = reinterpret_cast<uint32_t *>(best + G * RB);

    const uint32_t tid = threadIdx.x, rp = tid % HP, g = tid / HP;
    const uint32_t row0 = blockIdx.x * RB;
    if (tid == 0) *nchanged = 0;
    nn_key_t bk0 = 0, bk1 = 0;  // below every key of a real centroid

    for (uint32_t t0 = 0; t0 < a.k; t0 += a.tile) {
        const uint32_t tk = a.k - t0 < a.tile ? a.k - t0 : a.tile;
        __syncthreads();  // the previous tile has been read
        for (uint32_t i = tid; i < tk * (Dp / 4); i += kKmThreads) {
            const uint32_t c = i / (Dp / 4), d4 = i % (Dp / 4);
            *reinterpret_cast<float4 *>(Cs + (size_t)c * Dp + 4 * d4) = nn_load4(a.C, a.k, a.D, t0 + c, 4 * d4);
        }
        for (uint32_t s0 = 0; s0 < tk; s0 += SW) {
            const uint32_t sk = tk - s0 < SW ? tk - s0 : SW;
            const uint32_t na = (sk + G - 1) / G;  // accumulators in use: the same for every thread of the workgroup
            float acc0[kKmAcc], acc1[kKmAcc];
            uint32_t coff[kKmAcc];
#pragma unroll
            for (int e = 0; e < (int)kKmAcc; e++) {
                acc0[e] = acc1[e] = 0.f;
                const uint32_t c = s0 + g + G * e;  // a slot past the tile scores the tile's last centroid again and is dropped below
                coff[e] = (c < tk ? c : tk - 1) * Dp;
            }
            float4 pre[PRE];
            km_load_rows<PRE>(pre, a.X, a.n, a.D, row0, 0, tid);
            for (uint32_t c = 0; c < nch; c++) {
                __syncthreads();  // the previous chunk has been read
#pragma unroll
                for (int i = 0; i < PRE; i++) {
                    const uint32_t idx = tid + kKmThreads * i;
                    *reinterpret_cast<float4 *>(Xs + (idx >> 3) * kNnStride + 4 * (idx & 7u)) = pre[i];
                }
                __syncthreads();  // (also: the tile's centroids are in place)
                if (c + 1 < nch) km_load_rows<PRE>(pre, a.X, a.n, a.D, row0, (c + 1) * kNnChunk, tid);  // the next chunk travels while this one is scored
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const float4 x0 = *reinterpret_cast<const float4 *>(Xs + rp * kNnStride + 4 * j);
                    const float4 x1 = *reinterpret_cast<const float4 *>(Xs + (rp + HP) * kNnStride + 4 * j);
#pragma unroll
                    for (int e = 0; e < (int)kKmAcc; e++) {
                        if ((uint32_t)e < na) {
                            const float4 cv = *reinterpret_cast<const float4 *>(Cs + coff[e] + c * kNnChunk + 4 * j);
                            float s = acc0[e], u = acc1[e], t;
                            t = x0.x - cv.x; s = __builtin_fmaf(t, t, s);
                            t = x0.y - cv.y; s = __builtin_fmaf(t, t, s);
                            t = x0.z - cv.z; s = __builtin_fmaf(t, t, s);
                            t = x0.w - cv.w; s = __builtin_fmaf(t, t, s);
                            t = x1.x - cv.x; u = __builtin_fmaf(t, t, u);
                            t = x1.y - cv.y; u = __builtin_fmaf(t, t, u);
                            t = x1.z - cv.z; u = __builtin_fmaf(t, t, u);
                            t = x1.w - cv.w; u = __builtin_fmaf(t, t, u);
                            acc0[e] = s;
                            acc1[e] = u;
                        }
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < (int)kKmAcc; e++) {
                const uint32_t c = s0 + g + G * e;
                if ((uint32_t)e < na && c < tk) {
                    const nn_key_t k0 = nn_make_key(-acc0[e], t0 + c), k1 = nn_make_key(-acc1[e], t0 + c);
                    bk0 = k0 > bk0 ? k0 : bk0;
                    bk1 = k1 > bk1 ? k1 : bk1;
                }
            }
        }
    }

    best[g * RB + rp] = bk0;
    best[g * RB + rp + HP] = bk1;
    __syncthreads();
    uint32_t moved = 0;
    for (uint32_t r = tid; r < (uint32_t)RB; r += kKmThreads) {
        const uint32_t v = row0 + r;
        if (v >= a.n) continue;
        nn_key_t m = best[r];
        for (uint32_t gg = 1; gg < G; gg++) m = best[gg * RB + r] > m ? best[gg * RB + r] : m;
        const uint32_t label = ~(uint32_t)m, u = (uint32_t)(m >> 32);
        const float s = u == 0 ? __builtin_nanf("") : __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
        if (a.labels[v] != label) moved++;
        a.labels[v] = label;
        a.dist[v] = 0.f - s;
    }
    if (moved) atomicAdd(nchanged, moved);
    __syncthreads();
    if (tid == 0 && *nchanged) atomicAdd(a.changed, *nchanged);
}

// ---- stable grouping by label: hist[b][c] = members of cluster c among the vertices of block b ...
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const uint32_t *labels, uint32_t n, uint32_t k, uint32_t *hist) {
    __shared__ uint32_t h[kKmMaxK];
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kKmSortBlock;
    for (uint32_t i = threadIdx.x; i < kKmSortBlock; i += blockDim.x)
        if (base + i < n) atomicAdd(&h[labels[base + i]], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) hist[(size_t)blockIdx.x * k + i] = h[i];
}

// ... becomes the members of c in the blocks before b; counts[c] = all members of c.  One workgroup per cluster.
__global__ __launch_bounds__(256) void kmeans_offsets_kernel(uint32_t *hist, uint32_t blocks, uint32_t k, uint32_t *counts) {
    __shared__ uint32_t s[256];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, per = (blocks + 255) / 256;
    const uint32_t lo = tid * per < blocks ? tid * per : blocks, hi = lo + per < blocks ? lo + per : blocks;
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; b++) sum += hist[(size_t)b * k + c];
    s[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) {
            const uint32_t t = s[i];
            s[i] = run;
            run += t;
        }
        counts[c] = run;
    }
    __syncthreads();
    uint32_t run = s[tid];
    for (uint32_t b = lo; b < hi; b++) {
        const uint32_t t = hist[(size_t)b * k + c];
        hist[(size_t)b * k + c] = run;
        run += t;
    }
}

// start[c]: where cluster c's members begin in `order`; pstart[c]: the index of its first piece of 64 members (k + 1 entries each)
__global__ __launch_bounds__(256) void kmeans_starts_kernel(const uint32_t *counts, uint32_t k, uint32_t *start, uint32_t *pstart) {
    __shared__ uint32_t s[kKmMaxK];
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) s[i] = counts[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0, prun = 0;
        for (uint32_t c = 0; c < k; c++) {
            start[c] = run;
            pstart[c] = prun;
            run += s[c];
            prun += (s[c] + kKmPiece - 1) / kKmPiece;
        }
        start[k] = run;
        pstart[k] = prun;
    }
}

// order[start[c] + rank of v among c's members] = v.  One wavefront per block of vertices, 64 at a time in ascending id; lanes of
// one label are ranked by their lane number, so the order does not depend on how LDS atomics would have been served.
__global__ __launch_bounds__(64) void kmeans_scatter_kernel(const uint32_t *labels, uint32_t n, uint32_t k, const uint32_t *hist,
                                                            const uint32_t *start, uint32_t *order) {
    __shared__ uint32_t pos[kKmMaxK];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < k; i += 64) pos[i] = start[i] + hist[(size_t)blockIdx.x * k + i];
    __syncthreads();
    for (uint32_t step = 0; step < kKmSortBlock / 64; step++) {
        const uint32_t v = blockIdx.x * kKmSortBlock + step * 64 + lane;
        const bool live = v < n;
        const uint32_t l = live ? labels[v] : 0xFFFFFFFFu;
        unsigned long long todo = __ballot(live);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t ll = (uint32_t)__shfl((int)l, leader);
            const unsigned long long mask = __ballot(live && l == ll);
            if (live && l == ll) order[pos[ll] + __popcll(mask & ((1ull << lane) - 1ull))] = v;
            __syncthreads();
            if ((int)lane == leader) pos[ll] += (uint32_t)__popcll(mask);
            __syncthreads();
            todo &= ~mask;
        }
    }
}

struct KmSumArgs {
    const float *X;
    const uint32_t *order, *start, *counts, *pstart;
    double *psum;  // [piece][D]
    uint32_t n, D, k, lanes;  // lanes per piece: a power of two, 1..64
};

// One piece of up to 64 members per lane group, lane = four dimensions (and four more every 4 * lanes), eight member rows loaded
// before the first addition; fp64, in member order.
__global__ __launch_bounds__(256) void kmeans_piece_sum_kernel(const KmSumArgs a) {
    const uint32_t piece = (blockIdx.x * kKmThreads + threadIdx.x) / a.lanes, lig = threadIdx.x % a.lanes;
    if (piece >= a.pstart[a.k]) return;
    uint32_t lo = 0, hi = a.k;  // the cluster whose pieces hold `piece`: the first c with pstart[c + 1] > piece
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.pstart[mid + 1] > piece) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t p = piece - a.pstart[lo], m0 = a.start[lo] + p * kKmPiece;
    const uint32_t left = a.counts[lo] - p * kKmPiece, cnt = left < kKmPiece ? left : kKmPiece;
    for (uint32_t d0 = 4 * lig; d0 < a.D; d0 += 4 * a.lanes) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (uint32_t i = 0; i < cnt; i += 8) {
            float4 x[8];
#pragma unroll
            for (int u = 0; u < 8; u++)  // a slot past the piece's end loads nothing and adds +0
                x[u] = nn_load4(a.X, a.n, a.D, i + u < cnt ? a.order[m0 + i + u] : 0xFFFFFFFFu, d0);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                s0 += (double)x[u].x;
                s1 += (double)x[u].y;
                s2 += (double)x[u].z;
                s3 += (double)x[u].w;
            }
        }
        double *o = a.psum + (size_t)piece * a.D + d0;
        o[0] = s0;
        if (d0 + 1 < a.D) o[1] = s1;
        if (d0 + 2 < a.D) o[2] = s2;
        if (d0 + 3 < a.D) o[3] = s3;
    }
}

// grid (k, ceil(D / 32)): C[c][d] = (float)(sum of c's piece sums in piece order / count); an empty cluster keeps its centroid.
// The sums travel through LDS 64 pieces at a time (all 256 threads load), 32 threads add.
__global__ __launch_bounds__(256) void kmeans_centroid_kernel(const double *psum, const uint32_t *counts, const uint32_t *pstart, uint32_t D,
                                                              float *C) {
    __shared__ double t[kKmSumTile][32];
    const uint32_t c = blockIdx.x, d0 = blockIdx.y * 32, tid = threadIdx.x;
    const uint32_t cnt = counts[c];
    if (cnt == 0) return;
    const uint32_t base = pstart[c], np = pstart[c + 1] - base;
    double sum = 0.0;
    for (uint32_t p0 = 0; p0 < np; p0 += kKmSumTile) {
        __syncthreads();
        for (uint32_t i = tid; i < kKmSumTile * 32; i += kKmThreads) {
            const uint32_t pp = i >> 5, dd = i & 31u;
            t[pp][dd] = (p0 + pp < np && d0 + dd < D) ? psum[(size_t)(base + p0 + pp) * D + d0 + dd] : 0.0;
        }
        __syncthreads();
        if (tid < 32)
#pragma unroll 16
            for (uint32_t pp = 0; pp < kKmSumTile; pp++) sum += t[pp][tid];  // + 0.0 behind the last piece
    }
    if (tid < 32 && d0 + tid < D) C[(size_t)c * D + d0 + tid] = (float)(sum / (double)cnt);
}

// part[p] = dist[64 p] + dist[64 p + 1] + ... in fp64, sequentially
__global__ void kmeans_inertia_piece_kernel(const float *dist, uint32_t n, double *part) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if ((size_t)p * kKmPiece >= n) return;
    const uint32_t lo = p * kKmPiece, hi = n - lo < kKmPiece ? n : lo + kKmPiece;
    double s = 0.0;
    for (uint32_t v = lo; v < hi; v++) s += (double)dist[v];
    part[p] = s;
}

// *out = part[0] + part[1] + ... sequentially; one workgroup, the parts staged through LDS 256 at a time
__global__ __launch_bounds__(256) void kmeans_inertia_reduce_kernel(const double *part, uint32_t parts, double *out) {
    __shared__ double s[256];
    double sum = 0.0;
    for (uint32_t p0 = 0; p0 < parts; p0 += 256) {
        __syncthreads();
        s[threadIdx.x] = p0 + threadIdx.x < parts ? part[p0 + threadIdx.x] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0)
#pragma unroll 16
            for (uint32_t i = 0; i < 256; i++) sum += s[i];
    }
    if (threadIdx.x == 0) *out = sum;
}

struct ModArgs {
    const uint32_t *rowptr, *colids, *labels;
    unsigned long long *tallies;  // [0] edges, [1 .. nc] inside, [1 + nc .. 2 nc] degree
    uint32_t n, nc, lds;          // lds: tally in LDS (2 nc words of dynamic LDS) and add to `tallies` once per workgroup
};

// The simple undirected graph's edges by community.  One wavefront per row (grid stride), lanes over the row's nonzeros: entry
// (u, v) is a new edge unless it repeats the entry before it, or u > v and row v holds u (then row v counts it).
__global__ __launch_bounds__(256) void modularity_kernel(const ModArgs a) {
    extern __shared__ uint32_t mod_smem[];
    __shared__ uint32_t wg_edges;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (a.lds)
        for (uint32_t i = threadIdx.x; i < 2 * a.nc; i += blockDim.x) mod_smem[i] = 0;
    if (threadIdx.x == 0) wg_edges = 0;
    __syncthreads();
    uint32_t edges = 0;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1], lu = a.labels[u];
        for (uint32_t p = lo + lane; p < hi; p += 64) {
            const uint32_t v = a.colids[p];
            if (p > lo && a.colids[p - 1] == v) continue;
            if (u > v && nn_is_neighbour(a.rowptr, a.colids, v, u)) continue;
            const uint32_t lv = a.labels[v];
            edges++;
            if (a.lds) {
                atomicAdd(&mod_smem[a.nc + lu], 1u);
                atomicAdd(&mod_smem[a.nc + lv], 1u);
                if (lu == lv) atomicAdd(&mod_smem[lu], 1u);
            } else {
                atomicAdd(a.tallies + 1 + a.nc + lu, 1ull);
                atomicAdd(a.tallies + 1 + a.nc + lv, 1ull);
                if (lu == lv) atomicAdd(a.tallies + 1 + lu, 1ull);
            }
        }
    }
    if (edges) atomicAdd(&wg_edges, edges);
    __syncthreads();
    if (threadIdx.x == 0 && wg_edges) atomicAdd(a.tallies, (unsigned long long)wg_edges);
    if (a.lds)
        for (uint32_t i = threadIdx.x; i < 2 * a.nc; i += blockDim.x)
            if (mod_smem[i]) atomicAdd(a.tallies + 1 + i, (unsigned long long)mod_smem[i]);
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_KMEANS_HIP_H_
