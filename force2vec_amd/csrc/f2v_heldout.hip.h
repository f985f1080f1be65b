// f2v_heldout.hip.h -- held-out link prediction on gfx950 (definitions in include/f2v.h: held-out link prediction).
//
// The edge split (integers only: a function of the CSR, frac, seed and ratio, whatever the launch shapes):
//   held_anchor_kernel   one wavefront per row (grid stride), lanes over the row: the neighbour of smallest (key, id), a
//                        lexicographic minimum over the wavefront by xor shuffles;
//   held_count_kernel    one wavefront per row: every nonzero decides "held" from its key and the two anchors (held_forest_count_kernel
//                        and held_forest_fill_kernel: from its key and its forest flag -- f2v_edge_split_connected, which does not
//                        run the anchor kernel); the row's kept
//                        nonzeros, q(u) and |N(u)| ("distinct" is "differs from its predecessor") by ballots, total'(u) by the rule;
//                        the call's sums go to 64-bit words, one integer atomic per wavefront and word;
//   link_scan_*_kernel   (f2v_linkpairs.hip.h) the three exclusive prefix sums: kept nonzeros, held pairs, negatives;
//   held_fill_kernel     one wavefront per row: kept nonzero k of the row goes to colids_train[offset(u) + k], held pair k to its place;
//   link_short_kernel / link_long_kernel (f2v_linkpairs.hip.h) draw the negatives through LinkArgs: s1 = SN, p = 0, total = total',
//                        half = 0 and M = 2^64 - 1, under which link_perm is the identity: no shuffle.
// Pair scores:
//   pair_score_kernel    one wavefront per 64 pairs (grid stride), 32 dimensions a round: the 128 rows' slices are loaded by the
//                        whole wavefront -- one load instruction is two rows' 128 contiguous bytes -- into an LDS tile of 128 x 33
//                        words (the odd stride keeps the 32 lanes of a ds_read_b32 group on 32 banks), then lane l runs pair l's
//                        fma chains over the slice from LDS.  Any D; 16.5 KiB of LDS and 64 lanes a workgroup.
// Ranking:
//   rank_key_kernel      score -> 64-bit key, ascending key == descending score (-0 = +0, NaN last);
//   (rocprim::radix_sort_pairs sorts the keys with the labels as payload)
//   rank_scan_*_kernel   inclusive cumulative ones over the sorted labels (tile sums, link_scan_top_kernel, the tiles again);
//   rank_group_kernel    a thread per position: the last item of a group finds the group's first by binary search, forms pos_g, neg_g,
//                        TP_g, FP_g, adds its share of concordant / tied / groups (integer atomics, one per wavefront and word) and
//                        stores term_g at its position;
//   rank_block_kernel    a thread per block of 1024 positions: the block's terms summed sequentially from +0;
//   rank_total_kernel    one thread: the block sums added in ascending order.
// Plain launches, no in-grid waits, no float atomics.
#ifndef F2V_HELDOUT_HIP_H_
#define F2V_HELDOUT_HIP_H_

#include "f2v.h"
#include "f2v_kernels.hip.h"
#include "f2v_linkpairs.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kHeldNone = 0xFFFFFFFFu;  // the anchor of a vertex without neighbours (ids are below n <= 2^32 - 1)
constexpr uint32_t kPairDims = 32;           // dimensions per round of pair_score_kernel
constexpr uint32_t kPairStride = 33;         // words per row of its LDS tile
constexpr uint32_t kRankBlock = 1024;        // positions per block of the average-precision sum (the definition's)

struct HeldArgs {
    const uint32_t *rowptr, *colids;
    uint32_t *anchor;                  // per vertex: anchor(u), kHeldNone where N(u) is empty
    const uint8_t *forest;             // f2v_edge_split_connected: per nonzero, its pair is in the greatest spanning forest (f2v_components.hip.h)
    uint32_t *kept, *q, *total;        // per vertex: nonzeros that stay, held pairs with v > u, negatives
    const unsigned long long *kept_at, *held_at;  // per vertex: the index of its first kept nonzero / held pair
    unsigned long long *sums;          // [0] edges, [1] candidates, [2] held, [3] kept nonzeros, [4] negatives, [5] capped
    uint32_t *rowptr_out, *colids_out, *held_u, *held_v;
    uint64_t se, T;                    // SE, the threshold of a candidate's key
    uint32_t n, ratio;
};

__device__ __forceinline__ uint64_t held_key(const HeldArgs &a, uint32_t u, uint32_t v) {
    const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
    return mix64(a.se ^ (((uint64_t)lo << 32) | hi));
}

// nonzero q = (u, v): FOREST = false the anchors protect (f2v_edge_split), true the spanning forest does (f2v_edge_split_connected)
template <bool FOREST>
__device__ __forceinline__ bool held_is(const HeldArgs &a, uint32_t u, uint32_t v, uint32_t q) {
    if (u == v || held_key(a, u, v) >= a.T) return false;
    if constexpr (FOREST) return a.forest[q] == 0;
    else return a.anchor[u] != v && a.anchor[v] != u;
}

__global__ __launch_bounds__(256) void held_anchor_kernel(const HeldArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        unsigned long long best = ~0ull;
        uint32_t who = kHeldNone;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            if (lane >= hi - q0) continue;
            const uint32_t v = a.colids[q0 + lane];
            if (v == u) continue;
            const unsigned long long k = held_key(a, u, v);
            if (k < best || (k == best && v < who)) {
                best = k;
                who = v;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long ok = __shfl_xor(best, d);
            const uint32_t ow = __shfl_xor(who, d);
            if (ok < best || (ok == best && ow < who)) {
                best = ok;
                who = ow;
            }
        }
        if (lane == 0) a.anchor[u] = who;
    }
}

template <bool FOREST>
__device__ __forceinline__ void held_count_rows(const HeldArgs &a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long edges = 0, cands = 0, held = 0, kept = 0, neg = 0, capped = 0;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        uint32_t nu = 0, pu = 0, cu = 0, qu = 0, ku = 0;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            const bool in = lane < hi - q0;
            const uint32_t q = q0 + lane, v = in ? a.colids[q] : 0u;
            const bool nb = in && v != u && (q == lo || a.colids[q - 1] != v), up = nb && v > u;
            const bool is = in && held_is<FOREST>(a, u, v, q);
            nu += (uint32_t)__popcll(__ballot(nb));
            pu += (uint32_t)__popcll(__ballot(up));
            cu += (uint32_t)__popcll(__ballot(up && held_key(a, u, v) < a.T));
            qu += (uint32_t)__popcll(__ballot(up && is));
            ku += (uint32_t)__popcll(__ballot(in && !is));
        }
        const unsigned long long want = (unsigned long long)a.ratio * qu, room = (a.n - 1u - nu) / 2u;
        const uint32_t total = (uint32_t)(want < room ? want : room);
        if (lane == 0) {
            a.kept[u] = ku;
            a.q[u] = qu;
            a.total[u] = total;
        }
        edges += pu;
        cands += cu;
        held += qu;
        kept += ku;
        neg += total;
        capped += room < want ? 1u : 0u;
    }
    if (lane == 0) {
        if (edges) atomicAdd(a.sums + 0, edges);
        if (cands) atomicAdd(a.sums + 1, cands);
        if (held) atomicAdd(a.sums + 2, held);
        if (kept) atomicAdd(a.sums + 3, kept);
        if (neg) atomicAdd(a.sums + 4, neg);
        if (capped) atomicAdd(a.sums + 5, capped);
    }
}

__global__ __launch_bounds__(256) void held_count_kernel(const HeldArgs a) { held_count_rows<false>(a); }
__global__ __launch_bounds__(256) void held_forest_count_kernel(const HeldArgs a) { held_count_rows<true>(a); }

template <bool FOREST>
__device__ __forceinline__ void held_fill_rows(const HeldArgs &a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        uint64_t kat = a.kept_at[u], hat = a.held_at[u];
        if (lane == 0) a.rowptr_out[u] = (uint32_t)kat;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            const bool in = lane < hi - q0;
            const uint32_t q = q0 + lane, v = in ? a.colids[q] : 0u;
            const bool is = in && held_is<FOREST>(a, u, v, q);
            const bool pos = is && v > u && (q == lo || a.colids[q - 1] != v);
            const unsigned long long keep = __ballot(in && !is), take = __ballot(pos);
            if (in && !is) a.colids_out[kat + link_lanes_below(keep)] = v;
            if (pos) {
                const uint64_t at = hat + link_lanes_below(take);
                a.held_u[at] = u;
                a.held_v[at] = v;
            }
            kat += (uint32_t)__popcll(keep);
            hat += (uint32_t)__popcll(take);
        }
    }
}

__global__ __launch_bounds__(256) void held_fill_kernel(const HeldArgs a) { held_fill_rows<false>(a); }
__global__ __launch_bounds__(256) void held_forest_fill_kernel(const HeldArgs a) { held_fill_rows<true>(a); }

// ---- pair scores ---------------------------------------------------------------------------------------------------------------
struct PairArgs {
    const float *X;
    const uint32_t *u, *v;
    float *out;
    uint32_t m, D;
};

template <int METRIC>
__global__ __launch_bounds__(64) void pair_score_kernel(const PairArgs a) {
    __shared__ float tile[128 * kPairStride];
    __shared__ uint32_t ids[128];
    const uint32_t lane = threadIdx.x, col = lane & 31u, half = lane >> 5;
    const uint32_t groups = (a.m + 63u) / 64u;
    for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint32_t i = g * 64u + lane;  // (m <= 2^32 - 64: checked by the host)
        const bool in = i < a.m;
        ids[lane] = in ? a.u[i] : 0u;
        ids[64 + lane] = in ? a.v[i] : 0u;
        nn_wave_sync();
        float dot = 0.f, nu = 0.f, nv = 0.f;
        for (uint32_t d0 = 0; d0 < a.D; d0 += kPairDims) {
            const uint32_t w = a.D - d0 < kPairDims ? a.D - d0 : kPairDims;
            if (col < w) {
#pragma unroll 8
                for (uint32_t r = half; r < 128; r += 2) tile[r * kPairStride + col] = a.X[(size_t)ids[r] * a.D + d0 + col];
            }
            nn_wave_sync();
            const float *qs = tile + lane * kPairStride, *cs = tile + (64 + lane) * kPairStride;
            for (uint32_t k = 0; k < w; k++) {
                const float x = qs[k], y = cs[k];
                if constexpr (METRIC == F2V_SIM_L2) {
                    const float t = x - y;
                    dot = __builtin_fmaf(t, t, dot);
                } else {
                    dot = __builtin_fmaf(x, y, dot);
                    if constexpr (METRIC == F2V_SIM_COSINE) {
                        nu = __builtin_fmaf(x, x, nu);
                        nv = __builtin_fmaf(y, y, nv);
                    }
                }
            }
            nn_wave_sync();  // (the tile is overwritten by the next round)
        }
        float s = dot;
        if constexpr (METRIC == F2V_SIM_L2) s = -s;
        if constexpr (METRIC == F2V_SIM_COSINE) {
            const float ru = nu == 0.f ? 0.f : 1.0f / __builtin_sqrtf(nu), rv = nv == 0.f ? 0.f : 1.0f / __builtin_sqrtf(nv);
            s = (s * ru) * rv;
        }
        s = s != s ? __builtin_nanf("") : s + 0.0f;  // as f2v_nearest_rows reports a score: one NaN, -0 and +0 one score
        if (in) a.out[i] = s;
    }
}

// ---- ranking --------------------------------------------------------------------------------------------------------------------
struct RankArgs {
    const double *scores;
    unsigned long long *keys;          // sorted: ascending key == descending score
    const uint8_t *labels;             // sorted with them
    uint32_t *cum;                     // ones among positions 0 .. i
    unsigned long long *tile;          // the scan's tile sums
    double *terms, *blocks, *ap_sum;
    unsigned long long *tallies;       // [0] concordant, [1] tied, [2] groups
    uint64_t negatives;                // N
    uint32_t m;
};

__global__ __launch_bounds__(256) void rank_key_kernel(const RankArgs a) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.m; i += gridDim.x * 256u) {
        const double s = a.scores[i];
        unsigned long long k = 0;  // NaN: below every number
        if (s == s) {
            k = (unsigned long long)__double_as_longlong(s + 0.0);  // -0 and +0 are one score
            k = (k >> 63) ? ~k : (k | 0x8000000000000000ull);
        }
        a.keys[i] = ~k;
    }
}

__device__ __forceinline__ unsigned long long rank_tile_load(const RankArgs &a, uint32_t b, unsigned long long x[4]) {
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t i = (uint64_t)b * kLinkScanTile + threadIdx.x * 4u + k;
        x[k] = i < a.m ? (unsigned long long)a.labels[i] : 0ull;
        sum += x[k];
    }
    return sum;
}

__global__ __launch_bounds__(256) void rank_scan_tile_kernel(const RankArgs a) {
    __shared__ unsigned long long s[256];
    unsigned long long x[4], sum;
    link_block_scan(rank_tile_load(a, blockIdx.x, x), s, &sum);
    if (threadIdx.x == 0) a.tile[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void rank_scan_apply_kernel(const RankArgs a) {
    __shared__ unsigned long long s[256];
    unsigned long long x[4], sum;
    unsigned long long at = a.tile[blockIdx.x] + link_block_scan(rank_tile_load(a, blockIdx.x, x), s, &sum);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t i = (uint64_t)blockIdx.x * kLinkScanTile + threadIdx.x * 4u + k;
        at += x[k];
        if (i < a.m) a.cum[i] = (uint32_t)at;
    }
}

__device__ __forceinline__ unsigned long long rank_wave_sum(unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__global__ __launch_bounds__(256) void rank_group_kernel(const RankArgs a) {
    unsigned long long conc = 0, tied = 0, groups = 0;
    const uint32_t rounds = (a.m + 255u) / 256u;
    for (uint32_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const uint64_t i = (uint64_t)r * 256u + threadIdx.x;
        if (i >= a.m) continue;
        const unsigned long long key = a.keys[i];
        double term = 0.0;
        if (i + 1 == a.m || a.keys[i + 1] != key) {
            uint64_t lo = 0, hi = i;  // the group's first position: the first key that is not smaller
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (a.keys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            const uint64_t tp = a.cum[i], before = lo ? a.cum[lo - 1] : 0u, pos = tp - before, neg = (i + 1 - lo) - pos, fp = i + 1 - tp;
            conc += pos * (a.negatives - fp);
            tied += pos * neg;
            groups += 1;
            term = ((double)pos * (double)tp) / (double)(i + 1);
        }
        a.terms[i] = term;
    }
    conc = rank_wave_sum(conc);
    tied = rank_wave_sum(tied);
    groups = rank_wave_sum(groups);
    if ((threadIdx.x & 63u) == 0) {
        if (conc) atomicAdd(a.tallies + 0, conc);
        if (tied) atomicAdd(a.tallies + 1, tied);
        if (groups) atomicAdd(a.tallies + 2, groups);
    }
}

__global__ __launch_bounds__(64) void rank_block_kernel(const RankArgs a, uint32_t blocks) {
    const uint32_t b = blockIdx.x * 64u + threadIdx.x;
    if (b >= blocks) return;
    const uint64_t lo = (uint64_t)b * kRankBlock, hi = lo + kRankBlock < a.m ? lo + kRankBlock : a.m;
    double sum = 0.0;
    for (uint64_t i = lo; i < hi; i++) sum += a.terms[i];
    a.blocks[b] = sum;
}

__global__ void rank_total_kernel(const RankArgs a, uint32_t blocks) {
    if (blockIdx.x || threadIdx.x) return;
    double sum = 0.0;
    for (uint32_t b = 0; b < blocks; b++) sum += a.blocks[b];
    *a.ap_sum = sum;
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_HELDOUT_HIP_H_
