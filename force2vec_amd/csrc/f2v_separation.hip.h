// f2v_separation.hip.h -- how well a labelling separates in the embedding space: the silhouette and the Davies-Bouldin score
// (include/f2v.h, "separation").
//
// The members of every cluster in ascending vertex id come from the stable counting sort of f2v_kmeans.hip.h, run over the labelled
// vertices only.  Then
//   separation_pair_kernel     one workgroup scores a block of RB sample rows against ONE span (up to 64 pieces of 64 members) of one
//                              cluster.  The tiling is kmeans_assign_kernel's: 16-byte loads, chunks of 32 dimensions staged in LDS, a
//                              lane owns TWO sample rows and eight candidates' accumulators, the candidates of a sweep are dealt round
//                              robin to the workgroup's 512 / RB lane groups.  Here BOTH sides stream (a sweep's candidates change with
//                              every sweep), the fp32 accumulators persist over the chunks (the ascending-d chain of f2v.h), and a
//                              lane's two rows lie interleaved in LDS, so that one 16-byte read brings (x0_d, x1_d, x0_d+1, x1_d+1) and
//                              the subtract / fma pair of the two rows is one packed fp32 instruction each.  The 64 distances of a piece
//                              meet in LDS and are added in member order by one owner thread per sample row, in fp64; the owner keeps the
//                              span's running sum and writes ONE double per (sample, span);
//   separation_finish_kernel   one thread per sample: a cluster's span sums added in span order, then a, b, s and the cluster of b;
//   separation_piece_kernel    s(i) in pieces of 64 samples (kmeans_inertia_reduce_kernel adds the pieces);
//   separation_scatter_kernel  Davies-Bouldin: one wavefront per piece of 64 members, the distances to the members' own centroid,
//                              added in member order;
//   separation_cluster_kernel  a cluster's piece sums in span order, divided by its member count.
// No float atomics anywhere, no result depends on a launch shape: every sum has the one order f2v.h writes down.
#ifndef F2V_SEPARATION_HIP_H_
#define F2V_SEPARATION_HIP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f2v_kmeans.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kSepThreads = 256;
constexpr uint32_t kSepAcc = 8;         // candidates a thread scores per sweep (for each of its two rows)
constexpr uint32_t kSepPiece = 64;      // F2V_SEPARATION_PIECE
constexpr uint32_t kSepSpan = 64;       // F2V_SEPARATION_SPAN
constexpr uint32_t kSepMaxK = 1024;     // F2V_SEPARATION_MAX_CLUSTERS
constexpr uint32_t kSepChunk = 32;      // dimensions staged per step
constexpr uint32_t kSepCStride = 36;    // floats per staged candidate row (ds_read_b128 without bank conflicts)
constexpr uint32_t kSepXStride = 68;    // floats per staged PAIR of sample rows: 32 dimensions x 2 rows interleaved, 4 of padding
constexpr uint32_t kSepDStride = 65;    // floats per sample row of the piece's distances

typedef float sep_f2 __attribute__((ext_vector_type(2)));

// Four dimensions of row v from d on.  The row is always a real one (the caller clamps), dimensions past D read dimension 0 and
// become zeros: the only condition is the chunk's own (the k-means note on guarded loads).
__device__ inline float4 sep_load4(const float *X, uint32_t D, uint32_t v, uint32_t d) {
    const float *p = X + (size_t)v * D;
    if ((D & 3u) == 0) {
        const float4 x = *reinterpret_cast<const float4 *>(p + (d < D ? d : 0));
        return d < D ? x : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float e[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float x = p[d + q < D ? d + q : 0];
        e[q] = d + q < D ? x : 0.f;
    }
    return make_float4(e[0], e[1], e[2], e[3]);
}

// What separation_pair_kernel and trust_rank_kernel (f2v_layout.hip.h) share: the sample block's vertex ids, a chunk's way from the
// registers into LDS, and the scoring of the staged chunk.  Thread `tid` loads rows (tid + 256 i) / 8 at dimensions q4 .. q4 + 3.
template <int XP>
__device__ __forceinline__ void sep_samples(const uint32_t *sid, uint32_t row0, uint32_t nq, uint32_t hp, uint32_t tid, uint32_t (&xv0)[XP], uint32_t (&xv1)[XP]) {
#pragma unroll
    for (int i = 0; i < XP; i++) {
        const uint32_t p = (tid + kSepThreads * i) >> 3, r0 = row0 + p, r1 = row0 + p + hp;
        xv0[i] = sid[r0 < nq ? r0 : nq - 1];
        xv1[i] = sid[r1 < nq ? r1 : nq - 1];
    }
}

template <int XP, int CP>
__device__ __forceinline__ void sep_stage(float *Xs, float *Cs, const float4 (&px0)[XP], const float4 (&px1)[XP], const float4 (&pc)[CP], uint32_t tid, uint32_t q4) {
#pragma unroll
    for (int i = 0; i < XP; i++) {
        float *o = Xs + ((tid + kSepThreads * i) >> 3) * kSepXStride + 2 * q4;
        *reinterpret_cast<float4 *>(o) = make_float4(px0[i].x, px1[i].x, px0[i].y, px1[i].y);
        *reinterpret_cast<float4 *>(o + 4) = make_float4(px0[i].z, px1[i].z, px0[i].w, px1[i].w);
    }
#pragma unroll
    for (int i = 0; i < CP; i++) *reinterpret_cast<float4 *>(Cs + ((tid + kSepThreads * i) >> 3) * kSepCStride + q4) = pc[i];
}

// acc[e] += the squared differences, over the staged chunk, of the lane's two rows (pair rp) and candidate g + G e of the sweep
template <uint32_t G>
__device__ __forceinline__ void sep_score(const float *Xs, const float *Cs, uint32_t rp, uint32_t g, sep_f2 (&acc)[kSepAcc]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float4 xa = *reinterpret_cast<const float4 *>(Xs + rp * kSepXStride + 8 * j);
        const float4 xb = *reinterpret_cast<const float4 *>(Xs + rp * kSepXStride + 8 * j + 4);
        const sep_f2 x0 = {xa.x, xa.y}, x1 = {xa.z, xa.w}, x2 = {xb.x, xb.y}, x3 = {xb.z, xb.w};
#pragma unroll
        for (int e = 0; e < (int)kSepAcc; e++) {
            const float4 cc = *reinterpret_cast<const float4 *>(Cs + (g + G * e) * kSepCStride + 4 * j);
            sep_f2 t, u = acc[e];
            t = x0 - cc.x; u = __builtin_elementwise_fma(t, t, u);
            t = x1 - cc.y; u = __builtin_elementwise_fma(t, t, u);
            t = x2 - cc.z; u = __builtin_elementwise_fma(t, t, u);
            t = x3 - cc.w; u = __builtin_elementwise_fma(t, t, u);
            acc[e] = u;
        }
    }
}

struct SepPairArgs {
    const float *X;              // n x D, the settled matrix
    const uint32_t *order;       // the labelled vertices in cluster order, ascending id inside a cluster
    const uint32_t *sid;         // this launch's samples (vertex ids)
    const uint32_t *span_start;  // per span: the place of its first member in `order` ...
    const uint32_t *span_cnt;    // ... and its members (1..4096)
    double *ws;                  // [span][chunk]: the span sums
    uint32_t D, nq, chunk, blocks;  // nq: samples of this launch, chunk: the stride of ws, blocks = ceil(nq / RB)
};

// grid spans x blocks (the sample blocks of one span are neighbours: they share the span's rows in L2), 256 threads = 512 / RB lane
// groups of RB / 2 lanes; lane = sample rows (rp, rp + RB / 2) of the block, group g scores candidates g, g + G, g + 2G ... of a sweep.
// A sample row past the launch's last reads the last sample, a candidate past the span's end reads the span's last member: both are
// scored like any other and never summed.
template <int RB>
__global__ __launch_bounds__(256) void separation_pair_kernel(const SepPairArgs a) {
    constexpr uint32_t HP = RB / 2, G = kSepThreads / HP, SW = G * kSepAcc;
    constexpr int XP = RB / 64;  // pairs of 16-byte loads of sample rows per thread and chunk
    constexpr int CP = SW / 32;  // 16-byte loads of candidate rows per thread and chunk
    __shared__ __attribute__((aligned(16))) float Xs[HP * kSepXStride];  // [pair][d][2]: one chunk of the sample block
    __shared__ __attribute__((aligned(16))) float Cs[SW * kSepCStride];  // [candidate][d]: one chunk of the sweep's candidates
    __shared__ float Ds[RB * kSepDStride];                               // [sample row][member of the piece]: a piece's distances

    const uint32_t tid = threadIdx.x, rp = tid % HP, g = tid / HP;
    const uint32_t span = blockIdx.x / a.blocks, row0 = (blockIdx.x % a.blocks) * RB;
    const uint32_t m0 = a.span_start[span], cnt = a.span_cnt[span];
    const uint32_t nch = (a.D + kSepChunk - 1) / kSepChunk, nsw = (cnt + SW - 1) / SW;
    const uint32_t q4 = 4 * (tid & 7u);

    uint32_t xv0[XP], xv1[XP], cv[CP], cvn[CP];
    sep_samples<XP>(a.sid, row0, a.nq, HP, tid, xv0, xv1);
    auto members = [&](uint32_t (&v)[CP], uint32_t sweep) {
#pragma unroll
        for (int i = 0; i < CP; i++) {
            const uint32_t m = sweep * SW + ((tid + kSepThreads * i) >> 3);
            v[i] = a.order[m0 + (m < cnt ? m : cnt - 1)];
        }
    };
    float4 px0[XP], px1[XP], pc[CP];
    auto load = [&](const uint32_t (&v)[CP], uint32_t d0) {
#pragma unroll
        for (int i = 0; i < XP; i++) {
            px0[i] = sep_load4(a.X, a.D, xv0[i], d0 + q4);
            px1[i] = sep_load4(a.X, a.D, xv1[i], d0 + q4);
        }
#pragma unroll
        for (int i = 0; i < CP; i++) pc[i] = sep_load4(a.X, a.D, v[i], d0 + q4);
    };
    members(cvn, 0);
    load(cvn, 0);

    double span_sum = 0.0;  // of the owner thread's sample row (tid < RB)
    for (uint32_t s = 0; s < nsw; s++) {
        sep_f2 acc[kSepAcc];
#pragma unroll
        for (int e = 0; e < (int)kSepAcc; e++) acc[e] = sep_f2{0.f, 0.f};
#pragma unroll
        for (int i = 0; i < CP; i++) cv[i] = cvn[i];
        members(cvn, s + 1 < nsw ? s + 1 : s);  // the next sweep's ids travel while this one is scored
        for (uint32_t c = 0; c < nch; c++) {
            __syncthreads();  // the previous chunk has been read
            sep_stage<XP, CP>(Xs, Cs, px0, px1, pc, tid, q4);
            __syncthreads();
            // the next chunk (or the next sweep's first) travels while this one is scored
            if (c + 1 < nch) load(cv, (c + 1) * kSepChunk);
            else if (s + 1 < nsw) load(cvn, 0);
            sep_score<G>(Xs, Cs, rp, g, acc);
        }
        const uint32_t in_piece = (s * SW) % kSepPiece;  // the sweep's first place in its piece
#pragma unroll
        for (int e = 0; e < (int)kSepAcc; e++) {
            Ds[rp * kSepDStride + in_piece + g + G * e] = __builtin_sqrtf(acc[e].x);  // hipcc's default: correctly rounded, subnormals kept
            Ds[(rp + HP) * kSepDStride + in_piece + g + G * e] = __builtin_sqrtf(acc[e].y);
        }
        if (in_piece + SW == kSepPiece || s + 1 == nsw) {  // the piece is complete (the same for the whole workgroup)
            __syncthreads();
            if (tid < (uint32_t)RB) {
                // The piece's members only: the loop ends at the last member, a stand-in's distance is never read.  Nothing is added
                // for it -- not even +0 -- so the sum is the definition's whatever its sign rules would do to a zero.
                const uint32_t first = (s * SW) / kSepPiece * kSepPiece, pc_cnt = cnt - first < kSepPiece ? cnt - first : kSepPiece;
                const float *dr = Ds + tid * kSepDStride;
                double ps = 0.0;
                if (pc_cnt == kSepPiece) {
#pragma unroll 16
                    for (uint32_t j = 0; j < kSepPiece; j++) ps += (double)dr[j];
                } else {
                    for (uint32_t j = 0; j < pc_cnt; j++) ps += (double)dr[j];
                }
                span_sum += ps;
            }
            // (the next write to Ds lies behind the two barriers of the next sweep's first chunk)
        }
    }
    if (tid < (uint32_t)RB && row0 + tid < a.nq) a.ws[(size_t)span * a.chunk + row0 + tid] = span_sum;
}

struct SepFinishArgs {
    const double *ws;        // [span][chunk]
    const uint32_t *slab;    // the samples' labels
    const uint32_t *counts;  // members per cluster
    const uint32_t *cspan;   // k + 1: a cluster's first span
    double *s;               // per sample
    uint32_t *other;         // per sample: the cluster of b
    uint32_t nq, chunk, k;
};

// a(i), b(i), s(i) of f2v.h from the span sums: one thread per sample, clusters ascending, a cluster's spans ascending
__global__ __launch_bounds__(256) void separation_finish_kernel(const SepFinishArgs f) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.nq) return;
    const uint32_t L = f.slab[i];
    double av = 0.0, b = 0.0;
    uint32_t o = 0xFFFFFFFFu;
    for (uint32_t c = 0; c < f.k; c++) {
        const uint32_t nc = f.counts[c];
        if (nc == 0) continue;
        double sum = 0.0;
        for (uint32_t t = f.cspan[c]; t < f.cspan[c + 1]; t++) sum += f.ws[(size_t)t * f.chunk + i];
        if (c == L) {
            av = sum / (double)(nc - 1);
        } else {
            const double m = sum / (double)nc;
            if (o == 0xFFFFFFFFu || m < b) {
                b = m;
                o = c;
            }
        }
    }
    const double mx = av > b ? av : b;
    f.s[i] = (f.counts[L] == 1 || mx == 0.0) ? 0.0 : (b - av) / mx;
    f.other[i] = o;
}

// part[p] = s[64 p] + s[64 p + 1] + ... sequentially from +0
__global__ void separation_piece_kernel(const double *s, uint32_t n, double *part) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if ((size_t)p * kSepPiece >= n) return;
    const uint32_t lo = p * kSepPiece, hi = n - lo < kSepPiece ? n : lo + kSepPiece;
    double sum = 0.0;
    for (uint32_t v = lo; v < hi; v++) sum += s[v];
    part[p] = sum;
}

struct SepScatterArgs {
    const float *X, *C;  // the matrix, the k x D centroids
    const uint32_t *order, *start, *counts, *pstart;  // of the counting sort (kmeans_starts_kernel)
    double *part;        // per piece: the sum of its members' distances to their centroid
    uint32_t D, k;
};

// grid pieces, one wavefront: the piece's 64 member rows pass through LDS in chunks of 32 dimensions (coalesced 16-byte loads), lane =
// member for the chain; a slot past the cluster's end reads the cluster's last member and is never summed.
__global__ __launch_bounds__(64) void separation_scatter_kernel(const SepScatterArgs a) {
    __shared__ __attribute__((aligned(16))) float Xs[kSepPiece * kSepCStride];
    __shared__ __attribute__((aligned(16))) float Cc[kSepChunk];
    __shared__ float Ds[kSepPiece];
    const uint32_t piece = blockIdx.x, lane = threadIdx.x;
    if (piece >= a.pstart[a.k]) return;
    uint32_t lo = 0, hi = a.k;  // the cluster whose pieces hold `piece`: the first c with pstart[c + 1] > piece
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.pstart[mid + 1] > piece) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t p = piece - a.pstart[lo], m0 = a.start[lo] + p * kSepPiece;
    const uint32_t left = a.counts[lo] - p * kSepPiece, cnt = left < kSepPiece ? left : kSepPiece;
    const uint32_t nch = (a.D + kSepChunk - 1) / kSepChunk, q4 = 4 * (lane & 7u);
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t m = 8 * i + (lane >> 3);
        v[i] = a.order[m0 + (m < cnt ? m : cnt - 1)];
    }
    float acc = 0.f;
    for (uint32_t c = 0; c < nch; c++) {
        float4 pre[8];
#pragma unroll
        for (int i = 0; i < 8; i++) pre[i] = sep_load4(a.X, a.D, v[i], c * kSepChunk + q4);
        const float4 pcen = sep_load4(a.C, a.D, lo, c * kSepChunk + q4);
        __syncthreads();  // the previous chunk has been read
#pragma unroll
        for (int i = 0; i < 8; i++) *reinterpret_cast<float4 *>(Xs + (8 * i + (lane >> 3)) * kSepCStride + q4) = pre[i];
        if (lane < 8) *reinterpret_cast<float4 *>(Cc + q4) = pcen;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float4 x = *reinterpret_cast<const float4 *>(Xs + lane * kSepCStride + 4 * j);
            const float4 cc = *reinterpret_cast<const float4 *>(Cc + 4 * j);
            float t;
            t = x.x - cc.x; acc = __builtin_fmaf(t, t, acc);
            t = x.y - cc.y; acc = __builtin_fmaf(t, t, acc);
            t = x.z - cc.z; acc = __builtin_fmaf(t, t, acc);
            t = x.w - cc.w; acc = __builtin_fmaf(t, t, acc);
        }
    }
    Ds[lane] = __builtin_sqrtf(acc);
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;
        for (uint32_t j = 0; j < cnt; j++) sum += (double)Ds[j];  // the members only: nothing is added for a stand-in
        a.part[piece] = sum;
    }
}

// S[c] = (a cluster's piece sums in spans of 64 pieces: a span added from +0, the spans added from +0) / count; 0 for an empty cluster
__global__ void separation_cluster_kernel(const double *part, const uint32_t *counts, const uint32_t *pstart, uint32_t k, double *S) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= k) return;
    const uint32_t lo = pstart[c], hi = pstart[c + 1];
    double total = 0.0;
    for (uint32_t s0 = lo; s0 < hi; s0 += kSepSpan) {
        const uint32_t s1 = hi - s0 < kSepSpan ? hi : s0 + kSepSpan;
        double span = 0.0;
        for (uint32_t p = s0; p < s1; p++) span += part[p];
        total += span;
    }
    S[c] = counts[c] ? total / (double)counts[c] : 0.0;
}

// order[i] = ids[order[i]]: the counting sort ran over the labelled vertices' places, here they become vertex ids again
__global__ void separation_ids_kernel(uint32_t *order, const uint32_t *ids, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) order[i] = ids[order[i]];
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_SEPARATION_HIP_H_
