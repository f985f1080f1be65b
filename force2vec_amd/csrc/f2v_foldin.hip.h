// f2v_foldin.hip.h -- fold-in of new vertices into a trained embedding on gfx950 (definition in include/f2v.h).
//
// A new vertex whose neighbours are all existing vertices is a row whose update reads only frozen rows: every new vertex is
// independent of every other one, and ALL of its epochs run inside one launch with its vector in registers.  Per epoch a vertex reads
// its list's rows and ns sample rows -- the same list every epoch, so the rows stay cache-hot -- and nothing is written before the end.
//   fold_init_kernel   the initial vectors of one chunk: the fp64 neighbour mean in list order, or the counter-based random vector
//                      (a thread per value);
//   fold_q_kernel      D a multiple of 4 up to 256, one vertex per quarter-wave in the step kernels' layout (LPI lanes x NB 16-byte
//                      blocks, 64 / LPI vertices per wavefront).  Per epoch: the list's rows four at a time, all four gathers in
//                      flight before the first interaction (the ids of the next four are requested behind them), then the ns sample
//                      rows -- their ids come from mix64, a lane evaluating one id of four and handing it round its quad -- then
//                      the update.  The interactions are the step kernels' own device functions (pair_update_q; option 5 where a
//                      group's sums fit the registers: pair_dist_q, shared_coef5, pair_apply5_q), so the bits are the step kernels'.
//                      (A resident form -- a vertex's list rows gathered once into LDS and reread there every epoch -- was built and
//                      measured 7-11 % slower than rereading them through the caches: profiles/foldin_time.txt.  It is not here.)
//   fold_kernel        every other D up to 512, one wavefront per vertex in the generic layout of step_kernel (load_row, pair_update).
// Plain launches on the handle's stream: no in-grid waits, no atomics, no inline assembly beyond what the reused helpers hold.
#ifndef F2V_FOLDIN_HIP_H_
#define F2V_FOLDIN_HIP_H_

#include "f2v.h"
#include "f2v_kernels.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kFoldGroup = 4;  // rows in flight per vertex

struct FoldArgs {
    const float *X;           // the settled matrix, n x D
    const uint32_t *rowptr;   // the call's lists: vertex v has ids[rowptr[v] .. rowptr[v + 1])
    const uint32_t *ids;
    const uint32_t *order;    // this launch's vertices (indices into the call), longest list first
    float *Y0;                // the chunk's initial vectors: vertex v at row v - q0 (written by fold_init_kernel or uploaded)
    float *Y;                 // the chunk's results, likewise
    const float *sm_table;
    uint64_t seed_mix;        // mix64(seed)
    uint64_t index_base;
    uint32_t n, D;
    uint32_t q0, count;       // first vertex of the chunk; vertices of this launch
    uint32_t iters, ns;
    float lr;
};

// s(Q, e, k) for k = first + lane offset: the caller adds the offset to `counter`
__device__ __forceinline__ uint32_t fold_sample(const FoldArgs &a, uint64_t counter) { return (uint32_t)(mix64(a.seed_mix ^ counter) % (uint64_t)a.n); }

// ---- initial vectors ---------------------------------------------------------------------------------------------------------
// kind: F2V_FOLD_INIT_MEAN or F2V_FOLD_INIT_RANDOM; unit: the sigmoid options' range [0, 1)
__global__ __launch_bounds__(256) void fold_init_kernel(const FoldArgs a, int kind, int unit) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)a.count * a.D) return;
    const uint32_t r = (uint32_t)(idx / a.D), d = (uint32_t)(idx % a.D), v = a.q0 + r;
    const uint32_t lo = a.rowptr[v], cnt = a.rowptr[v + 1] - lo;
    float y;
    if (kind == F2V_FOLD_INIT_MEAN && cnt != 0u) {
        double s = 0.0;
        for (uint32_t k = 0; k < cnt; ++k) s = s + (double)a.X[(size_t)a.ids[lo + k] * a.D + d];
        y = (float)(s / (double)cnt);
    } else {
        const uint64_t Q = a.index_base + v;
        const float u = (float)(uint32_t)(mix64(a.seed_mix ^ ((1ull << 63) | (Q * a.D + d))) >> 40) * 0x1p-24f;
        y = unit ? u : 2.0f * u - 1.0f;
    }
    a.Y0[(size_t)r * a.D + d] = y;
}

// ---- quarter-wave layout -----------------------------------------------------------------------------------------------------
// Four rows of one item against x_i (option 5): their sums, ONE evaluation of the four coefficients, then the first `live`
// contributions onto Y in order.  A slot past `live` holds a real row; its coefficient is dropped, never multiplied.
template <int LPI, int NB, bool NEG>
__device__ __forceinline__ void fold_quad5(const float (&xi)[NB][4], const float4 (&xj)[kFoldGroup][NB], uint32_t live, uint32_t t, float (&Y)[NB][4], float lr) {
    f32x2_t d[kFoldGroup][NB][2];
    float sum[kFoldGroup], cf[kFoldGroup];
#pragma unroll
    for (uint32_t u = 0; u < kFoldGroup; ++u) sum[u] = pair_dist_q<LPI, NB>(xi, xj[u], d[u]);
    shared_coef5<4, NEG>(sum, lane_sel<4>(t), cf);
#pragma unroll
    for (uint32_t u = 0; u < kFoldGroup; ++u) {
        if (u < live) pair_apply5_q<NB>(d[u], Y, lr, cf[u]);
    }
}

// the first `live` of four gathered rows applied onto Y in order
template <int OPT, int LPI, int NB, bool NEG>
__device__ __forceinline__ void fold_apply_q(const float (&xi)[NB][4], const float4 (&xj)[kFoldGroup][NB], uint32_t live, uint32_t t, float (&Y)[NB][4], float lr,
                                             double c0, const float *table) {
    if constexpr (OPT == 5 && NB <= 2) {
        fold_quad5<LPI, NB, NEG>(xi, xj, live, t, Y, lr);
    } else {
#pragma unroll
        for (uint32_t u = 0; u < kFoldGroup; ++u) {
            if (u < live) pair_update_q<OPT, LPI, NB, NEG>(xi, xj[u], Y, lr, c0, table);
        }
    }
}

// lane t's pieces of row j of the matrix (a dead piece -- past D -- is the tree's zero padding)
template <int LPI, int NB, bool FULL>
__device__ __forceinline__ void fold_load_q(const float *X, uint32_t j, uint32_t t, uint32_t D, float4 (&out)[NB]) {
    const float *src = X + (size_t)j * D;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if constexpr (FULL) {
            out[b] = *reinterpret_cast<const float4 *>(src + t * 4 + 4 * LPI * b);
        } else {
            const bool live = 4u * LPI * b + 4u * t < D;  // (a dead piece reads the row's first 16 bytes and drops them)
            const float4 v = *reinterpret_cast<const float4 *>(src + (live ? t * 4 + 4 * LPI * b : 0u));
            out[b] = live ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <int OPT, int LPI, int NB, bool FULL>
__global__ __launch_bounds__(256) void fold_q_kernel(const FoldArgs a) {
    constexpr uint32_t DP = 4u * LPI * NB, IPW = 64u / LPI;  // padded dims (the tree's width); vertices per wavefront
    static_assert(LPI >= 4, "a quad of lanes shares the sample ids and option 5's coefficients");
    extern __shared__ __attribute__((aligned(16))) char fold_lds[];
    const uint32_t D = FULL ? DP : a.D;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = lane & (LPI - 1u), q = lane / LPI;
    const uint32_t wpb = blockDim.x >> 6;
    // the sigmoid options look their table up once per interaction: from LDS (as qstep_body has it)
    float *sm_lds = reinterpret_cast<float *>(fold_lds);
    if constexpr (OPT != 5) {
        for (uint32_t k = threadIdx.x; k < 2048u; k += blockDim.x) sm_lds[k] = a.sm_table[k];
        __syncthreads();
    }
    const float *table = OPT == 5 ? a.sm_table : sm_lds;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + (threadIdx.x >> 6)));
    if (IPW * w >= a.count) return;

    // this item's lanes (lane groups past the end of the launch idle on the wavefront's first vertex with an empty list and store nothing)
    const uint32_t slot = IPW * w + q;
    const bool active = slot < a.count;
    const uint32_t v = a.order[active ? slot : IPW * w];
    const uint32_t lo = a.rowptr[v], deg = a.rowptr[v + 1] - lo;
    const uint32_t cnt = active ? deg : 0u;
    const uint32_t maxcnt = wave_max_of_items<LPI>(cnt);
    const uint32_t last = cnt != 0u ? cnt - 1u : 0u;
    const uint32_t *list = a.ids + lo;
    const uint64_t Q = a.index_base + v;

    float xi[NB][4], Y[NB][4];
    {
        float4 y0[NB];
        fold_load_q<LPI, NB, FULL>(a.Y0, v - a.q0, t, D, y0);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            xi[b][0] = y0[b].x; xi[b][1] = y0[b].y; xi[b][2] = y0[b].z; xi[b][3] = y0[b].w;
        }
    }
    double c0 = 0.0;
    if constexpr (OPT != 5) {
        const float degi = (float)(1.0 / (double)(deg + 1u));  // algorithms.cpp:854, deg = the list's length
        c0 = (double)(a.lr * degi);
    }

    for (uint32_t e = 0; e < a.iters; ++e) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int c = 0; c < 4; ++c) Y[b][c] = OPT == 5 ? 0.0f : xi[b][c];  // the sigmoid options accumulate onto a copy of the vector

        // the list, in the caller's order.  Every slot of a group loads a row unconditionally (a branch around a load serialises the
        // group's gathers): a slot past the list's end reads its last row again, an empty list row 0 -- nothing outside the matrix.
        uint32_t j[kFoldGroup];
#pragma unroll
        for (uint32_t u = 0; u < kFoldGroup; ++u) j[u] = cnt != 0u ? list[u < last ? u : last] : 0u;
        for (uint32_t g = 0; g < maxcnt; g += kFoldGroup) {
            float4 xj[kFoldGroup][NB];
#pragma unroll
            for (uint32_t u = 0; u < kFoldGroup; ++u) fold_load_q<LPI, NB, FULL>(a.X, j[u], t, D, xj[u]);
#pragma unroll
            for (uint32_t u = 0; u < kFoldGroup; ++u) {
                const uint32_t k = g + kFoldGroup + u;
                j[u] = cnt != 0u ? list[k < last ? k : last] : 0u;
            }
            asm volatile("" ::: "memory");  // (keeps the gathers above the predicated interactions, as qprocess does)
            fold_apply_q<OPT, LPI, NB, false>(xi, xj, cnt > g ? cnt - g : 0u, t, Y, a.lr, c0, table);
        }

        // the negative samples s(Q, e, 0 .. ns-1): lane t evaluates the id of sample k0 + (t & 3), its quad hands the four round
        // (an id past ns - 1 is a vertex all the same: its row is gathered and dropped)
        const uint64_t counter = (Q * a.iters + e) * a.ns;
        for (uint32_t k0 = 0; k0 < a.ns; k0 += kFoldGroup) {
            const int mine = (int)fold_sample(a, counter + k0 + (t & 3u));
            uint32_t sj[kFoldGroup];
            sj[0] = (uint32_t)__builtin_amdgcn_update_dpp(0, mine, 0x00, 0xF, 0xF, true);
            sj[1] = (uint32_t)__builtin_amdgcn_update_dpp(0, mine, 0x55, 0xF, 0xF, true);
            sj[2] = (uint32_t)__builtin_amdgcn_update_dpp(0, mine, 0xAA, 0xF, 0xF, true);
            sj[3] = (uint32_t)__builtin_amdgcn_update_dpp(0, mine, 0xFF, 0xF, 0xF, true);
            float4 xs[kFoldGroup][NB];
#pragma unroll
            for (uint32_t u = 0; u < kFoldGroup; ++u) fold_load_q<LPI, NB, FULL>(a.X, sj[u], t, D, xs[u]);
            fold_apply_q<OPT, LPI, NB, true>(xi, xs, a.ns - k0, t, Y, a.lr, c0, table);
        }

#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int c = 0; c < 4; ++c) xi[b][c] = OPT == 5 ? xi[b][c] + Y[b][c] : Y[b][c];  // algorithms.cpp:636 / :918
        if constexpr (!FULL) {
            // a dead piece must stay the tree's zero padding for the next epoch: where a pair's sum is 0 (a sample that equals the
            // vector) the coefficient is inf, and 0 x inf = NaN scales to -5 in the dead dims as in the live ones.  The step kernels
            // never see it: they load x_i afresh in every launch and store live dims only.
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (!(4u * LPI * b + 4u * t < D)) xi[b][0] = xi[b][1] = xi[b][2] = xi[b][3] = 0.0f;
            }
        }
    }

    if (active) {
        float *out = a.Y + (size_t)(v - a.q0) * D + t * 4;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (!FULL && !(4u * LPI * b + 4u * t < D)) continue;
            *reinterpret_cast<float4 *>(out + 4 * LPI * b) = make_float4(xi[b][0], xi[b][1], xi[b][2], xi[b][3]);
        }
    }
}

// ---- generic layout: one wavefront per vertex ----------------------------------------------------------------------------------
// `cnt` rows named by id_at(k), k < cnt, against x_i in order: 64 ids per round (one per lane), 8 row gathers in flight (process_list)
template <int OPT, int VEC, bool EXACT, bool NEG, class IdAt>
__device__ __forceinline__ void fold_walk(const FoldArgs &a, uint32_t cnt, uint32_t lane, const float (&xi)[VEC], float (&Y)[VEC], double c0, IdAt id_at) {
    constexpr int U = 8;
    for (uint32_t base = 0; base < cnt; base += 64u) {
        const uint32_t c = (cnt - base) < 64u ? (cnt - base) : 64u;
        const uint32_t idv = lane < c ? id_at(base + lane) : 0u;
        for (uint32_t g = 0; g < c; g += U) {
            float xj[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t k = (g + u) < c ? (g + u) : (c - 1u);
                const uint32_t j = (uint32_t)__builtin_amdgcn_readlane((int)idv, (int)k);
                load_row<VEC, EXACT>(a.X + (size_t)j * a.D, lane, a.D, xj[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (g + u < c) pair_update<OPT, VEC, NEG>(xi, xj[u], Y, a.lr, c0, a.sm_table);
            }
        }
    }
}

template <int OPT, int VEC, bool EXACT>
__global__ __launch_bounds__(256) void fold_kernel(const FoldArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + (threadIdx.x >> 6)));
    if (w >= a.count) return;
    const uint32_t v = a.order[w];
    const uint32_t lo = a.rowptr[v], cnt = a.rowptr[v + 1] - lo;
    const uint64_t Q = a.index_base + v;
    float xi[VEC], Y[VEC];
    load_row<VEC, EXACT>(a.Y0 + (size_t)(v - a.q0) * a.D, lane, a.D, xi);
    double c0 = 0.0;
    if constexpr (OPT != 5) {
        const float degi = (float)(1.0 / (double)(cnt + 1u));  // algorithms.cpp:854
        c0 = (double)(a.lr * degi);
    }
    for (uint32_t e = 0; e < a.iters; ++e) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) Y[c] = OPT == 5 ? 0.0f : xi[c];
        fold_walk<OPT, VEC, EXACT, false>(a, cnt, lane, xi, Y, c0, [&](uint32_t k) { return a.ids[lo + k]; });
        const uint64_t counter = (Q * a.iters + e) * a.ns;
        fold_walk<OPT, VEC, EXACT, true>(a, a.ns, lane, xi, Y, c0, [&](uint32_t k) { return fold_sample(a, counter + k); });
#pragma unroll
        for (int c = 0; c < VEC; ++c) xi[c] = OPT == 5 ? xi[c] + Y[c] : Y[c];
        if constexpr (!EXACT) {  // (the dims past D stay zero padding: see fold_q_kernel)
#pragma unroll
            for (int c = 0; c < VEC; ++c)
                if (lane * VEC + c >= a.D) xi[c] = 0.0f;
        }
    }
    store_row<VEC, EXACT>(a.Y + (size_t)(v - a.q0) * a.D, lane, a.D, xi);
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v

#endif  // F2V_FOLDIN_HIP_H_
