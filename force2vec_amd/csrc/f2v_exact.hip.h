// f2v_exact.hip.h -- the exact all-pairs Force2Vec (option 1) on gfx950: training step and objective (definition in include/f2v.h).
//
// Every row of a minibatch is repelled by all n vertices, so the work is n x rows x D arithmetic on (n + rows) x D floats: the
// columns are staged through LDS once per workgroup and every staged value serves all of the workgroup's rows.
//   exact_pair_q_kernel    the pair kernel for D a multiple of 4 up to 256 and minibatches of "exact_quarter_min" rows or more, in the step kernels' quarter-wave layout (four rows per wavefront on
//                          the DPP rows, their tree reduction and their shared fp64 coefficient evaluation): see its own comment.
//   exact_pair_kernel      the pair kernel for every other D, for smaller minibatches and with "quarter_wave" = 0.  grid = (groups of rows of the minibatch) x (spans + 1).  A workgroup is four wavefronts, a wavefront holds
//                          RW rows of the minibatch in registers in the generic layout of step_kernel (lane l owns dims [l*VEC, +VEC),
//                          the pair sum is wave_allreduce_tree(inlane_tree): the adjacent-pair tree over next_pow2(D) zero-padded
//                          terms), with a piece sum and a span sum per row beside them.  Slice s < spans walks the columns of span s,
//                          piece by piece, out of LDS; the same lanes own the same (row, d) throughout, so the definition's order needs
//                          no cross-wave combination.  The fp64 coefficients of 64 / RW columns x RW rows are evaluated together, one
//                          per lane, and read back with v_readlane: one fp64 evaluation serves 64 pairs.  The extra slice s == spans walks
//                          the rows' CSR neighbours (the attraction part A), four row gathers in flight.
//   exact_finish_kernel    Y = A + S_0 + S_1 ... in order, x_i += Y in place: the pair kernel has finished by then, and this kernel
//                          reads only the workspace and the row itself.
//   exact_objective_kernel the same tiling over all n columns per group of rows: lane c of a wavefront keeps the pair sum of the
//                          piece's c-th column, so one fp64 evaluation of the two logs serves 64 pairs; piece and row sums in the
//                          definition's order.  exact_objective_reduce_kernel adds the row sums in pieces of 64 rows.
// No atomics, no in-grid waits, no inline assembly beyond what the reused helpers hold.
#ifndef F2V_EXACT_HIP_H_
#define F2V_EXACT_HIP_H_

#include "f2v.h"
#include "f2v_kernels.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kExactPiece = F2V_EXACT_PIECE;                     // columns per piece
constexpr uint32_t kExactSpanCols = F2V_EXACT_PIECE * F2V_EXACT_SPAN;  // columns per span
static_assert(kExactPiece == 64, "a piece is one column per lane of a wavefront (exact_objective_kernel)");

struct ExactArgs {
    float *X;  // the matrix: read as it was before the minibatch by the pair kernel, rows [lo, hi) updated in place by the finish kernel
    const uint32_t *rowptr, *colids;
    float *ws;  // (hi - lo) x (spans + 1) x D: row r's span sums S_0 .. S_(spans-1), then its attraction part A
    uint32_t n, D, lo, hi, spans;
    float step;
};

struct ExactObjArgs {
    const float *X;
    const uint32_t *rowptr, *colids;
    double *row_att, *row_rep;  // n each
    uint32_t n, D;
};

// columns staged at a time: rows of 64 * VEC (zero-padded) floats, 16 KB (VEC = 1) or 32 KB of LDS
template <int VEC> constexpr int kExactStage = VEC <= 2 ? 64 : 128 / VEC;

// the columns [first, first + cnt) of X as zero-padded rows of 64 * VEC floats (cnt <= kExactStage<VEC>, first + cnt <= n)
template <int VEC>
__device__ __forceinline__ void exact_stage(float *s_col, const float *X, uint32_t first, uint32_t cnt, uint32_t D) {
    constexpr uint32_t W = 64u * VEC;
    if (D % 4u == 0u) {  // rows are 16-byte aligned: 16-byte loads
        for (uint32_t idx = threadIdx.x; idx < cnt * (W / 4u); idx += blockDim.x) {
            const uint32_t c = idx / (W / 4u), d = 4u * (idx % (W / 4u));
            const float4 v = d < D ? *reinterpret_cast<const float4 *>(X + (size_t)(first + c) * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(s_col + c * W + d) = v;
        }
    } else {
        for (uint32_t idx = threadIdx.x; idx < cnt * W; idx += blockDim.x) {
            const uint32_t c = idx / W, d = idx % W;
            s_col[idx] = d < D ? X[(size_t)(first + c) * D + d] : 0.0f;
        }
    }
}

template <int VEC>
__device__ __forceinline__ void exact_lds_row(const float *s_col, uint32_t c, uint32_t lane, float (&out)[VEC]) {
    load_vec<VEC>(s_col + c * (64u * VEC) + lane * VEC, out);
}

__device__ __forceinline__ float exact_readlane(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// the repulsion's coefficient (sample/algorithms.cpp:402, :417)
__device__ __forceinline__ float exact_d_rep(float a) { return (float)(2.0 / ((double)a * (1.0 + (double)a))); }

template <int VEC, bool EXACT, int RW>
__global__ __launch_bounds__(256) void exact_pair_kernel(const ExactArgs a) {
    constexpr int STAGE = kExactStage<VEC>;
    constexpr int G = (64 / RW) < STAGE ? 64 / RW : STAGE;  // columns whose coefficients are evaluated together
    __shared__ __attribute__((aligned(16))) float s_col[STAGE * 64 * VEC];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (a scalar: so are the row ids)
    const uint32_t D = a.D, n = a.n;
    const uint32_t row0 = a.lo + (blockIdx.x * 4u + wave) * RW;
    uint32_t rid[RW];
    float xi[RW][VEC];
#pragma unroll
    for (int r = 0; r < RW; ++r) {  // a row past the minibatch computes on its last row and stores nothing
        rid[r] = row0 + r;
        load_row<VEC, EXACT>(a.X + (size_t)(rid[r] < a.hi ? rid[r] : a.hi - 1u) * D, lane, D, xi[r]);
    }
    const uint32_t s = blockIdx.y;
    const size_t slots = (size_t)a.spans + 1u;
    if (s < a.spans) {
        float S[RW][VEC];
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int v = 0; v < VEC; ++v) S[r][v] = 0.0f;
        const uint32_t c_begin = s * kExactSpanCols;
        const uint32_t c_end = (n - c_begin) < kExactSpanCols ? n : c_begin + kExactSpanCols;
        for (uint32_t pb = c_begin; pb < c_end; pb += kExactPiece) {
            const uint32_t pe = (c_end - pb) < kExactPiece ? c_end : pb + kExactPiece;
            float P[RW][VEC];
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int v = 0; v < VEC; ++v) P[r][v] = 0.0f;
            for (uint32_t sb = pb; sb < pe; sb += STAGE) {  // (every bound here depends on the workgroup's slice alone: the barriers are uniform)
                const uint32_t cnt = (pe - sb) < (uint32_t)STAGE ? pe - sb : (uint32_t)STAGE;
                __syncthreads();  // the columns staged before have been read
                exact_stage<VEC>(s_col, a.X, sb, cnt, D);
                __syncthreads();
                // G columns at a time: first their RW pair sums each -- lane k * RW + r keeps that of column k and row r --, then ONE
                // fp64 evaluation of all G * RW coefficients, then the additions in column order (the differences are taken again)
                for (uint32_t g0 = 0; g0 < cnt; g0 += G) {
                    const uint32_t gc = (cnt - g0) < (uint32_t)G ? cnt - g0 : (uint32_t)G;
                    float mine = 1.0f;  // (a lane without a pair evaluates a finite coefficient nobody reads)
#pragma unroll
                    for (int k = 0; k < G; ++k) {
                        if ((uint32_t)k < gc) {
                            float xj[VEC];
                            exact_lds_row<VEC>(s_col, g0 + k, lane, xj);
#pragma unroll
                            for (int r = 0; r < RW; ++r) {
                                float t[VEC];
#pragma unroll
                                for (int v = 0; v < VEC; ++v) {
                                    const float d = xi[r][v] - xj[v];
                                    t[v] = d * d;
                                }
                                const float sum = wave_allreduce_tree(inlane_tree<VEC>(t));
                                mine = (lane == (uint32_t)(k * RW + r)) ? sum : mine;
                            }
                        }
                    }
                    const float cf = exact_d_rep(mine);
#pragma unroll
                    for (int k = 0; k < G; ++k) {
                        if ((uint32_t)k < gc) {
                            float xj[VEC];
                            exact_lds_row<VEC>(s_col, g0 + k, lane, xj);
                            const uint32_t col = sb + g0 + k;
#pragma unroll
                            for (int r = 0; r < RW; ++r) {
                                if (col != rid[r]) {  // (uniform: the row ids and the column are the wavefront's)
                                    const float d1 = exact_readlane(cf, k * RW + r);
#pragma unroll
                                    for (int v = 0; v < VEC; ++v) {
                                        const float f = clamp_ref((xi[r][v] - xj[v]) * d1);
                                        const float p = a.step * f;
                                        P[r][v] = P[r][v] + p;
                                    }
                                }
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int v = 0; v < VEC; ++v) S[r][v] = S[r][v] + P[r][v];
        }
#pragma unroll
        for (int r = 0; r < RW; ++r)
            if (rid[r] < a.hi) store_row<VEC, EXACT>(a.ws + ((size_t)(rid[r] - a.lo) * slots + s) * D, lane, D, S[r]);
    } else {  // the attraction part: the rows' CSR neighbours in row order (sample/algorithms.cpp:378-393)
        constexpr uint32_t U = 4;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            if (rid[r] >= a.hi) continue;
            float A[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) A[v] = 0.0f;
            const uint32_t nb = a.rowptr[rid[r]], ne = a.rowptr[rid[r] + 1u];
            for (uint32_t e = nb; e < ne; e += U) {
                float xj[U][VEC];
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    const uint32_t j = a.colids[e + u < ne ? e + u : ne - 1u];
                    load_row<VEC, EXACT>(a.X + (size_t)j * D, lane, D, xj[u]);
                }
#pragma unroll
                for (uint32_t u = 0; u < U; ++u) {
                    if (e + u >= ne) break;
                    float diff[VEC], t[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        diff[v] = xi[r][v] - xj[u][v];
                        t[v] = diff[v] * diff[v];
                    }
                    const float sum = wave_allreduce_tree(inlane_tree<VEC>(t));
                    const float d1 = (float)(-2.0 / (1.0 + (double)sum));
                    const float d2 = exact_d_rep(sum);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float f = clamp_ref(diff[v] * d1) - clamp_ref(diff[v] * d2);
                        const float p = a.step * f;
                        A[v] = A[v] + p;
                    }
                }
            }
            store_row<VEC, EXACT>(a.ws + ((size_t)(rid[r] - a.lo) * slots + a.spans) * D, lane, D, A);
        }
    }
}

// The pair kernel in the step kernels' quarter-wave layout, for D a multiple of 4 up to 256: a wavefront holds FOUR rows of the
// minibatch, one per DPP row -- lane t of a row's 16 owns dims [64 b + 4 t, +4) of block b < NB --, so every VALU instruction serves
// four (row, column) pairs and the pair sum needs four DPP steps per block and neither the LDS crossbar nor an SGPR hop.  It reuses
// the step kernels' pair_dist_q (differences, squares, the tree), shared_coef5 (ONE fp64 evaluation of four columns' coefficients
// per row on a quad of lanes) and pair_apply5_q.  The same operations on the same values in the same order as exact_pair_kernel:
// the same bits.  A workgroup is one, two or four wavefronts ("exact_rows" 4, 8, 16).
template <int NB>
__device__ __forceinline__ void exact_lds_row_q(const float *s_col, uint32_t c, uint32_t t, float4 (&out)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) out[b] = *reinterpret_cast<const float4 *>(s_col + c * (64u * NB) + 64u * b + 4u * t);
}

template <int NB>
__device__ __forceinline__ void exact_store_q(float *dst, uint32_t t, uint32_t D, const float (&in)[NB][4]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint32_t d0 = 64u * b + 4u * t;
        if (d0 < D) *reinterpret_cast<float4 *>(dst + d0) = make_float4(in[b][0], in[b][1], in[b][2], in[b][3]);
    }
}

template <int NB>
__global__ __launch_bounds__(256) void exact_pair_q_kernel(const ExactArgs a) {
    constexpr int STAGE = kExactStage<NB>;
    constexpr int U = 4;  // columns whose coefficients a quad of lanes evaluates together
    __shared__ __attribute__((aligned(16))) float s_col[STAGE * 64 * NB];
    const uint32_t t = threadIdx.x & 15u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t D = a.D, n = a.n;
    const uint32_t row0 = a.lo + (blockIdx.x * (blockDim.x >> 6) + wave) * 4u;  // the wavefront's first row (a scalar)
    const uint32_t rid = row0 + ((threadIdx.x >> 4) & 3u);
    const bool live = rid < a.hi;  // a row past the minibatch computes on its last row and stores nothing
    float xi[NB][4];
    obj_load<NB, false>(a.X + (size_t)(live ? rid : a.hi - 1u) * D, t, D, xi);
    const uint32_t s = blockIdx.y;
    const size_t slots = (size_t)a.spans + 1u;
    if (s < a.spans) {
        const LaneSel<4> sel = lane_sel<4>(t);
        float S[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) S[b][v] = 0.0f;
        const uint32_t c_begin = s * kExactSpanCols;
        const uint32_t c_end = (n - c_begin) < kExactSpanCols ? n : c_begin + kExactSpanCols;
        for (uint32_t pb = c_begin; pb < c_end; pb += kExactPiece) {
            const uint32_t pe = (c_end - pb) < kExactPiece ? c_end : pb + kExactPiece;
            float P[NB][4];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < 4; ++v) P[b][v] = 0.0f;
            for (uint32_t sb = pb; sb < pe; sb += STAGE) {
                const uint32_t cnt = (pe - sb) < (uint32_t)STAGE ? pe - sb : (uint32_t)STAGE;
                __syncthreads();
                exact_stage<NB>(s_col, a.X, sb, cnt, D);
                __syncthreads();
                for (uint32_t g = 0; g < cnt; g += U) {
                    f32x2_t d[U][NB][2];
                    float sum[U], cf[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {  // (a column past the staged ones stands in with the last one: its coefficient is dropped)
                        float4 xj4[NB];
                        exact_lds_row_q<NB>(s_col, g + u < cnt ? g + u : cnt - 1u, t, xj4);
                        sum[u] = pair_dist_q<16, NB>(xi, xj4, d[u]);
                    }
                    shared_coef5<4, true>(sum, sel, cf);
                    const uint32_t col = sb + g;
                    if (col + U <= row0 || col >= row0 + 4u) {  // (uniform) none of the four columns is one of the wavefront's rows
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (g + u < cnt) pair_apply5_q<NB>(d[u], P, a.step, cf[u]);
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if (g + u < cnt) {
                                float Q[NB][4];
#pragma unroll
                                for (int b = 0; b < NB; ++b)
#pragma unroll
                                    for (int v = 0; v < 4; ++v) Q[b][v] = P[b][v];
                                pair_apply5_q<NB>(d[u], Q, a.step, cf[u]);
                                const bool other = col + u != rid;  // j == i is skipped
#pragma unroll
                                for (int b = 0; b < NB; ++b)
#pragma unroll
                                    for (int v = 0; v < 4; ++v) P[b][v] = other ? Q[b][v] : P[b][v];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int v = 0; v < 4; ++v) S[b][v] = S[b][v] + P[b][v];
        }
        if (live) exact_store_q<NB>(a.ws + ((size_t)(rid - a.lo) * slots + s) * D, t, D, S);
    } else {  // the attraction part: every DPP row walks its own row's CSR neighbours, as long as the longest of the four
        float A[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int v = 0; v < 4; ++v) A[b][v] = 0.0f;
        const uint32_t nb = live ? a.rowptr[rid] : 0u, deg = live ? a.rowptr[rid + 1u] - nb : 0u;
        for (uint32_t e = 0; __any(e < deg); ++e) {
            const bool mine = e < deg;
            const uint32_t j = mine ? a.colids[nb + e] : (live ? rid : a.hi - 1u);
            float xj[NB][4];
            obj_load<NB, false>(a.X + (size_t)j * D, t, D, xj);
            float4 xj4[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) xj4[b] = make_float4(xj[b][0], xj[b][1], xj[b][2], xj[b][3]);
            f32x2_t d[NB][2];
            const float sum = pair_dist_q<16, NB>(xi, xj4, d);
            const float d1 = coef5<false>(sum), d2 = coef5<true>(sum);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float dv = (v & 1) ? d[b][v >> 1].y : d[b][v >> 1].x;
                    const float f = clamp_ref(dv * d1) - clamp_ref(dv * d2);
                    const float p = a.step * f;
                    const float q = A[b][v] + p;
                    A[b][v] = mine ? q : A[b][v];
                }
            }
        }
        if (live) exact_store_q<NB>(a.ws + ((size_t)(rid - a.lo) * slots + a.spans) * D, t, D, A);
    }
}

// One thread per (row, d) of the minibatch
__global__ __launch_bounds__(256) void exact_finish_kernel(const ExactArgs a) {
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
    const size_t total = (size_t)(a.hi - a.lo) * a.D;
    if (idx >= total) return;
    const size_t r = idx / a.D, d = idx % a.D;
    const size_t slots = (size_t)a.spans + 1u;
    const float *w = a.ws + r * slots * a.D + d;
    float Y = w[(size_t)a.spans * a.D];
    for (uint32_t s = 0; s < a.spans; ++s) Y = Y + w[(size_t)s * a.D];
    float *x = a.X + (size_t)a.lo * a.D + idx;
    *x = *x + Y;
}

// ---- the exact objective ---------------------------------------------------------------------------------------------------------
// flog of include/f2v.h: the natural logarithm of a positive normal fp64 number from additions, multiplications and one division in
// a stated order (the algorithm of fdlibm's e_log.c without its special cases), so that a host restatement reproduces its bits.
__device__ __forceinline__ double exact_flog(double x) {
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, x);
    int k = (int)((bits >> 52) & 0x7FFull) - 1023;
    double m = __builtin_bit_cast(double, (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);  // [1, 2)
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        k += 1;
    }
    const double f = m - 1.0;
    const double dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double R = t2 + t1;
    const double hfsq = (0.5 * f) * f;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

__device__ __forceinline__ double exact_readlane64(double v, uint32_t lane) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// the sequential sum, from +0, of the first `cnt` lanes' terms: every lane receives it
__device__ __forceinline__ double exact_lane_chain(double term, uint32_t cnt) {
    double p = 0.0;
    for (uint32_t k = 0; k < cnt; ++k) p = p + exact_readlane64(term, k);
    return p;
}

template <int VEC, bool EXACT>
__global__ __launch_bounds__(256) void exact_objective_kernel(const ExactObjArgs a) {
    constexpr int STAGE = kExactStage<VEC>;
    constexpr int RW = 4;
    __shared__ __attribute__((aligned(16))) float s_col[STAGE * 64 * VEC];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t D = a.D, n = a.n;
    const uint32_t row0 = (blockIdx.x * 4u + wave) * RW;
    uint32_t rid[RW];
    float xi[RW][VEC];
    double rep[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        rid[r] = row0 + r;
        rep[r] = 0.0;
        load_row<VEC, EXACT>(a.X + (size_t)(rid[r] < n ? rid[r] : n - 1u) * D, lane, D, xi[r]);
    }
    for (uint32_t pb = 0; pb < n; pb += kExactPiece) {
        const uint32_t pe = (n - pb) < kExactPiece ? n : pb + kExactPiece;
        float mine[RW];  // the pair sums of column pb + lane
#pragma unroll
        for (int r = 0; r < RW; ++r) mine[r] = 0.0f;
        for (uint32_t sb = pb; sb < pe; sb += STAGE) {
            const uint32_t cnt = (pe - sb) < (uint32_t)STAGE ? pe - sb : (uint32_t)STAGE;
            __syncthreads();
            exact_stage<VEC>(s_col, a.X, sb, cnt, D);
            __syncthreads();
            for (uint32_t c = 0; c < cnt; ++c) {
                float xj[VEC];
                exact_lds_row<VEC>(s_col, c, lane, xj);
                const bool here = lane == (sb - pb) + c;
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    float t[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float d = xi[r][v] - xj[v];
                        t[v] = d * d;
                    }
                    const float sum = wave_allreduce_tree(inlane_tree<VEC>(t));
                    mine[r] = here ? sum : mine[r];
                }
            }
        }
        const uint32_t col = pb + lane;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const double z = (double)mine[r];
            const double term = (col < pe && col != rid[r]) ? -(exact_flog(1e-6 + z) - exact_flog(1.0 + z)) : 0.0;
            rep[r] = rep[r] + exact_lane_chain(term, pe - pb);
        }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        if (rid[r] >= n) continue;
        double att = 0.0;
        const uint32_t nb = a.rowptr[rid[r]], ne = a.rowptr[rid[r] + 1u];
        for (uint32_t pb = nb; pb < ne; pb += kExactPiece) {
            const uint32_t cnt = (ne - pb) < kExactPiece ? ne - pb : kExactPiece;
            float mine = 0.0f;
            for (uint32_t c = 0; c < cnt; ++c) {
                float xj[VEC], t[VEC];
                load_row<VEC, EXACT>(a.X + (size_t)a.colids[pb + c] * D, lane, D, xj);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float d = xi[r][v] - xj[v];
                    t[v] = d * d;
                }
                const float sum = wave_allreduce_tree(inlane_tree<VEC>(t));
                mine = (lane == c) ? sum : mine;
            }
            const double term = lane < cnt ? exact_flog(1.0 + (double)mine) : 0.0;
            att = att + exact_lane_chain(term, cnt);
        }
        if (lane == 0) {
            a.row_att[rid[r]] = att;
            a.row_rep[rid[r]] = rep[r];
        }
    }
}

// One workgroup: the row sums in pieces of 64 consecutive rows (sequentially from +0), then the piece sums sequentially.
// piece: 2 x ceil(n / 64) doubles of workspace.
__global__ __launch_bounds__(1024) void exact_objective_reduce_kernel(const double *row_att, const double *row_rep, uint32_t n, unsigned long long nnz,
                                                                      double *piece, ObjPartial *out) {
    const uint32_t pieces = (n + kExactPiece - 1u) / kExactPiece;
    for (uint32_t p = threadIdx.x; p < pieces; p += 1024u) {
        const uint32_t lo = p * kExactPiece, hi = (n - lo) < kExactPiece ? n : lo + kExactPiece;
        double att = 0.0, rep = 0.0;
        for (uint32_t r = lo; r < hi; ++r) {
            att = att + row_att[r];
            rep = rep + row_rep[r];
        }
        piece[p] = att;
        piece[pieces + p] = rep;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double att = 0.0, rep = 0.0;
        for (uint32_t p = 0; p < pieces; ++p) {
            att = att + piece[p];
            rep = rep + piece[pieces + p];
        }
        *out = ObjPartial{att, rep, nnz, (unsigned long long)n * (n - 1u)};
    }
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif
