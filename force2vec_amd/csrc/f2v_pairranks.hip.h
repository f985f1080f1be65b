// f2v_pairranks.hip.h -- filtered ranks of pairs on gfx950 (include/f2v.h, "ranks of pairs").
//
// For a pair (u, v): how many rows of the matrix are more similar to row u than row v is, how many tie with it -- counted over all n
// rows without storing a score, then corrected for the rows the flags exclude.  Three plain launches per chunk of pairs:
//   pair_score_kernel    (f2v_heldout.hip.h) the targets t = s(u, v): the definition's bits by construction;
//   prank_count_kernel   the base counts over ALL n rows.  The launch has the shape of nearest_kernel: grid (query blocks, splits), 256
//                        threads = WQ x (4 / WQ) wavefronts of MI x NI tiles of 32 queries x 32 candidates; the query block (row u of
//                        every pair, gathered by nearest_gather_kernel) resident in LDS, candidate tiles of 128 staged through
//                        nn_load4 / nn_store4 with the next chunk of 32 dimensions prefetched; dot and cosine on
//                        v_mfma_f32_32x32x2_f32, whose accumulator is the fma chain, L2 on the vector ALU in that accumulator's
//                        layout.  Where nearest_kernel selects, this kernel compares W(score) with the query row's W(t) and counts,
//                        per lane, in registers, across all tiles of its split; at the end the 32 candidate lanes of a query row are
//                        added by xor shuffles, the workgroup's candidate wavefronts through two words per query row in LDS, and
//                        every (pair, split) adds once to the pair's two counters.  Candidates at or past n and query rows past the
//                        chunk's end count for nothing (a zero-padded candidate row scores 0 under dot: it would beat every
//                        negative target).  LDS: the query block, one candidate tile, four words per query row;
//   prank_correct_kernel one wavefront per work item -- (pair, piece of 256 nonzeros of CSR row u), or the pair itself: u under
//                        EXCLUDE_SELF and v, which the base pass counted as a tie with itself.  The distinct members of E are scored
//                        against row u by the fma chain of pair_score_kernel (64 member rows a round, 32 dimensions a step, through
//                        an LDS tile of 65 x 33 words) and what ranked above or tied is subtracted; the members are counted for
//                        `candidates`.  A hub's row is many items: a pair (hub, v) does not serialise on one wavefront.
// W(s) is the high word of nn_make_key.  The only atomics are integer additions (a subtraction adds the two's complement), so the two
// counters of a pair cannot depend on the order in which splits, workgroups or items land.  No in-grid waits.
#ifndef F2V_PAIRRANKS_HIP_H_
#define F2V_PAIRRANKS_HIP_H_

#include "f2v.h"
#include "f2v_nearest.hip.h"
#include "f2v_heldout.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kPrankPiece = 256;              // nonzeros of row u per work item of the correction
constexpr uint32_t kPrankPairItem = 0xFFFFFFFFu;   // PrankItem::piece of the item that stands for the pair itself

struct PrankItem {
    uint32_t pair, piece;  // index of the pair in its chunk; piece of row u, or kPrankPairItem
};

struct PrankArgs {
    const float *X;              // n x D, the settled matrix
    const float *Q;              // nq x D: row u of every pair of the chunk
    const float *rc;             // cosine: 1 / |x| per row of X; nullptr otherwise
    const float *t;              // per pair: the target's score s(u, v)
    const uint32_t *u, *v;       // per pair
    const uint32_t *rowptr, *colids;
    const PrankItem *item;
    uint32_t *greater, *equal;   // per pair
    unsigned long long *excluded;  // the chunk's sum of |E|
    uint32_t n, D, nq, flags, tiles_per_split, items;
};

// the order-preserving image of a score: NaN 0, -0 and +0 one word
__device__ inline uint32_t prank_word(float s) { return (uint32_t)(nn_make_key(s, 0u) >> 32); }

__host__ __device__ inline size_t prank_lds_bytes(uint32_t qb, uint32_t D) {
    const size_t nch = (D + kNnChunk - 1) / kNnChunk;
    return (nch * qb * kNnStride + (size_t)kNnTile * kNnStride) * sizeof(float) + (size_t)4 * qb * sizeof(uint32_t);
}

// grid (query blocks, splits), 256 threads = WQ x (4 / WQ) wavefronts, each MI x NI tiles of 32 queries x 32 candidates
template <bool L2, int WQ, int MI, int NI>
__global__ __launch_bounds__(256) void prank_count_kernel(const PrankArgs a) {
    constexpr int WC = 4 / WQ;
    constexpr uint32_t QB = 32u * WQ * MI;
    static_assert(32u * WC * NI == kNnTile, "a workgroup's wavefronts cover one candidate tile");
    extern __shared__ float4 prank_smem[];
    const uint32_t nch = (a.D + kNnChunk - 1) / kNnChunk;
    float *Qs = reinterpret_cast<float *>(prank_smem);  // [chunk][query][kNnStride]
    float *Cs = Qs + (size_t)nch * QB * kNnStride;      // [candidate][kNnStride]
    uint32_t *wts = reinterpret_cast<uint32_t *>(Cs + kNnTile * kNnStride);  // W(t) of the query row
    float *rqs = reinterpret_cast<float *>(wts + QB);
    uint32_t *sum = reinterpret_cast<uint32_t *>(rqs + QB);  // [query][greater, equal] of this workgroup

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t wq = wave / WC, wc = wave % WC;
    const uint32_t q0 = blockIdx.x * QB, split = blockIdx.y;
    const uint32_t tiles = (a.n + kNnTile - 1) / kNnTile;
    const uint32_t tile_lo = split * a.tiles_per_split;
    const uint32_t tile_hi = tile_lo + a.tiles_per_split < tiles ? tile_lo + a.tiles_per_split : tiles;
    const bool cosine = a.rc != nullptr;

    for (uint32_t i = tid; i < QB; i += kNnThreads) {
        const bool live = q0 + i < a.nq;
        wts[i] = live ? prank_word(a.t[q0 + i]) : 0u;
        rqs[i] = cosine && live ? a.rc[a.u[q0 + i]] : 0.f;
        sum[2 * i] = sum[2 * i + 1] = 0u;
    }
    for (uint32_t i = tid; i < QB * nch * 8u; i += kNnThreads) {
        const uint32_t row = i / (nch * 8u), c = (i % (nch * 8u)) >> 3, c4 = i & 7u;
        nn_store4(Qs + ((size_t)c * QB + row) * kNnStride, c4, nn_load4(a.Q, a.nq, a.D, q0 + row, c * kNnChunk + 4 * c4));
    }
    __syncthreads();

    // accumulator (mi, ni, e) of this lane is query row (e & 3) + 8 (e >> 2) + 4 h of tile mi, candidate column r of tile ni
    uint32_t gt[MI][16], eq[MI][16];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int e = 0; e < 16; e++) gt[mi][e] = eq[mi][e] = 0u;

    for (uint32_t tile = tile_lo; tile < tile_hi; tile++) {
        const uint32_t cb = tile * kNnTile;
        nn_f32x16 acc[MI][NI];
#pragma unroll
        for (int mi = 0; mi < MI; mi++)
#pragma unroll
            for (int ni = 0; ni < NI; ni++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[mi][ni][e] = 0.f;

        float4 pre[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t idx = tid + kNnThreads * i;
            pre[i] = nn_load4(a.X, a.n, a.D, cb + (idx >> 3), 4 * (idx & 7u));
        }
        for (uint32_t c = 0; c < nch; c++) {
            __syncthreads();  // the previous chunk has been read
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t idx = tid + kNnThreads * i;
                nn_store4(Cs + (idx >> 3) * kNnStride, idx & 7u, pre[i]);
            }
            __syncthreads();
            if (c + 1 < nch) {  // the next chunk travels while this one is multiplied
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t idx = tid + kNnThreads * i;
                    pre[i] = nn_load4(a.X, a.n, a.D, cb + (idx >> 3), (c + 1) * kNnChunk + 4 * (idx & 7u));
                }
            }
            const float *Qc = Qs + (size_t)c * QB * kNnStride;
            if constexpr (!L2) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float4 av[MI], bv[NI];
#pragma unroll
                    for (int mi = 0; mi < MI; mi++)
                        av[mi] = *reinterpret_cast<const float4 *>(Qc + ((wq * MI + mi) * 32u + r) * kNnStride + 16 * h + 4 * j);
#pragma unroll
                    for (int ni = 0; ni < NI; ni++)
                        bv[ni] = *reinterpret_cast<const float4 *>(Cs + ((wc * NI + ni) * 32u + r) * kNnStride + 16 * h + 4 * j);
#pragma unroll
                    for (int e = 0; e < 4; e++)
#pragma unroll
                        for (int mi = 0; mi < MI; mi++)
#pragma unroll
                            for (int ni = 0; ni < NI; ni++) {
                                const float qa = e == 0 ? av[mi].x : e == 1 ? av[mi].y : e == 2 ? av[mi].z : av[mi].w;
                                const float cv = e == 0 ? bv[ni].x : e == 1 ? bv[ni].y : e == 2 ? bv[ni].z : bv[ni].w;
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa, cv, acc[mi][ni], 0, 0, 0);
                            }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float4 ce[NI], co[NI];
#pragma unroll
                    for (int ni = 0; ni < NI; ni++) {
                        const float *cr = Cs + ((wc * NI + ni) * 32u + r) * kNnStride + 4 * j;
                        ce[ni] = *reinterpret_cast<const float4 *>(cr);
                        co[ni] = *reinterpret_cast<const float4 *>(cr + 16);
                    }
#pragma unroll
                    for (int mi = 0; mi < MI; mi++)
#pragma unroll
                        for (int e = 0; e < 16; e++) {
                            const uint32_t qrow = (wq * MI + mi) * 32u + (e & 3) + 8 * (e >> 2) + 4 * h;
                            const float *qr = Qc + qrow * kNnStride + 4 * j;
                            const float4 qe = *reinterpret_cast<const float4 *>(qr);
                            const float4 qo = *reinterpret_cast<const float4 *>(qr + 16);
#pragma unroll
                            for (int ni = 0; ni < NI; ni++) {
                                float s = acc[mi][ni][e], t;
                                t = qe.x - ce[ni].x; s = __builtin_fmaf(t, t, s);
                                t = qo.x - co[ni].x; s = __builtin_fmaf(t, t, s);
                                t = qe.y - ce[ni].y; s = __builtin_fmaf(t, t, s);
                                t = qo.y - co[ni].y; s = __builtin_fmaf(t, t, s);
                                t = qe.z - ce[ni].z; s = __builtin_fmaf(t, t, s);
                                t = qo.z - co[ni].z; s = __builtin_fmaf(t, t, s);
                                t = qe.w - ce[ni].w; s = __builtin_fmaf(t, t, s);
                                t = qo.w - co[ni].w; s = __builtin_fmaf(t, t, s);
                                acc[mi][ni][e] = s;
                            }
                        }
                }
            }
        }

        // ---- counting: a candidate at or past n (the zero padding of the last tile) is nobody's rival
#pragma unroll
        for (int ni = 0; ni < NI; ni++) {
            const uint32_t cand = cb + (wc * NI + ni) * 32u + r;
            if (cand >= a.n) continue;
            const float rcv = cosine ? a.rc[cand] : 0.f;
#pragma unroll
            for (int mi = 0; mi < MI; mi++)
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const uint32_t qrow = (wq * MI + mi) * 32u + (e & 3) + 8 * (e >> 2) + 4 * h;
                    float s = acc[mi][ni][e];
                    if constexpr (L2) s = -s;
                    else if (cosine) s = (s * rqs[qrow]) * rcv;
                    const uint32_t w = prank_word(s), wt = wts[qrow];
                    gt[mi][e] += w > wt ? 1u : 0u;
                    eq[mi][e] += w == wt ? 1u : 0u;
                }
        }
    }

    // ---- a query row's 32 candidate lanes, then the workgroup's candidate wavefronts, then one addition per (pair, split)
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            uint32_t g = gt[mi][e], q = eq[mi][e];
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) {
                g += __shfl_xor(g, d);
                q += __shfl_xor(q, d);
            }
            if (r == 0) {
                const uint32_t qrow = (wq * MI + mi) * 32u + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (g) atomicAdd(&sum[2 * qrow], g);
                if (q) atomicAdd(&sum[2 * qrow + 1], q);
            }
        }
    __syncthreads();
    for (uint32_t i = tid; i < QB; i += kNnThreads) {
        if (q0 + i >= a.nq) continue;  // a row past the chunk's end counted zero rows of Q: it has no counters
        if (sum[2 * i]) atomicAdd(&a.greater[q0 + i], sum[2 * i]);
        if (sum[2 * i + 1]) atomicAdd(&a.equal[q0 + i], sum[2 * i + 1]);
    }
}

// One wavefront per work item (the host launches a workgroup per item; a smaller grid strides).  METRIC: F2V_SIM_*.
template <int METRIC>
__global__ __launch_bounds__(64) void prank_correct_kernel(const PrankArgs a) {
    __shared__ float tile[65 * kPairStride];  // 64 member rows' slices, then row u's
    __shared__ uint32_t ids[64];
    const uint32_t lane = threadIdx.x, col = lane & 31u, half = lane >> 5;
    const bool self = (a.flags & F2V_NEAREST_EXCLUDE_SELF) != 0;
    unsigned long long excluded = 0;
    for (uint32_t it = blockIdx.x; it < a.items; it += gridDim.x) {
        const PrankItem item = a.item[it];
        const uint32_t i = item.pair, u = a.u[i], v = a.v[i], wt = prank_word(a.t[i]);
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        const bool whole = item.piece == kPrankPairItem;
        const uint32_t rounds = whole ? 1u : kPrankPiece / 64u;
        uint32_t g = 0, e = whole ? 1u : 0u, members = 0;  // v itself: the base pass counted it, and it ties with itself (a NaN too)
        for (uint32_t round = 0; round < rounds; round++) {
            bool member;
            uint32_t w = u;
            if (whole) {
                member = lane == 0 && self && u != v;
            } else {
                const uint64_t p0 = (uint64_t)lo + (uint64_t)item.piece * kPrankPiece + round * 64u;
                if (p0 >= hi) break;
                const uint64_t p = p0 + lane;
                member = p < hi;
                if (member) {  // a duplicated nonzero counts once; v stays a target; u is the pair item's under EXCLUDE_SELF
                    w = a.colids[p];
                    member = (p == lo || a.colids[p - 1] != w) && w != v && !(self && w == u);
                }
            }
            const unsigned long long live = __ballot(member);
            if (!live) continue;
            ids[lane] = w;  // (a lane without a member holds a vertex all the same: u, or the nonzero it turned down)
            nn_wave_sync();
            float dot = 0.f;
            for (uint32_t d0 = 0; d0 < a.D; d0 += kPairDims) {
                const uint32_t wd = a.D - d0 < kPairDims ? a.D - d0 : kPairDims;
                if (col < wd) {
#pragma unroll 8
                    for (uint32_t row = half; row < 64; row += 2) tile[row * kPairStride + col] = a.X[(size_t)ids[row] * a.D + d0 + col];
                    if (half == 0) tile[64 * kPairStride + col] = a.X[(size_t)u * a.D + d0 + col];
                }
                nn_wave_sync();
                const float *qs = tile + 64 * kPairStride, *cs = tile + lane * kPairStride;
                for (uint32_t k = 0; k < wd; k++) {
                    const float x = qs[k], y = cs[k];
                    if constexpr (METRIC == F2V_SIM_L2) {
                        const float t = x - y;
                        dot = __builtin_fmaf(t, t, dot);
                    } else {
                        dot = __builtin_fmaf(x, y, dot);
                    }
                }
                nn_wave_sync();  // (the tile is overwritten by the next step, the ids by the next round)
            }
            float s = dot;
            if constexpr (METRIC == F2V_SIM_L2) s = -s;
            if constexpr (METRIC == F2V_SIM_COSINE) s = (s * a.rc[u]) * a.rc[w];
            const uint32_t ww = prank_word(s);
            g += (uint32_t)__popcll(__ballot(member && ww > wt));
            e += (uint32_t)__popcll(__ballot(member && ww == wt));
            members += (uint32_t)__popcll(live);
        }
        if (lane == 0) {
            if (g) atomicAdd(&a.greater[i], 0u - g);
            if (e) atomicAdd(&a.equal[i], 0u - e);
        }
        excluded += members;
    }
    if (lane == 0 && excluded) atomicAdd(a.excluded, excluded);
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_PAIRRANKS_HIP_H_
