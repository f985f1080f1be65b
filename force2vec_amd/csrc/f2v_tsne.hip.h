// f2v_tsne.hip.h -- exact t-SNE of the embedding over a sparse neighbour affinity matrix: f2v_tsne_affinities and f2v_tsne
// (definition in include/f2v.h, "t-SNE layout").
//
// The state of an iteration is Y, update and gains (m x d2 doubles) and yf = (float)Y (m x d2 floats, two copies: the step kernel
// reads one and writes the other).  One iteration is four plain launches on the handle's stream:
//   tsne_pair_kernel       the hot path, the n-body loop.  grid = (row blocks, slices of whole spans).  A lane owns one row: its yf and
//                          the running piece sums live in registers.  The workgroup stages one span of columns (16 pieces of 64) in
//                          LDS, component by component; every lane reads the same address (a broadcast), walks a piece in ascending j
//                          -- the definition's order, no cross-lane combination -- adds the piece sums in fp64 into the span sums and
//                          stores those to the workspace [span][component][row].  Only a piece that holds one of the workgroup's own
//                          rows pays for the j == i test.  A row slot past m computes on row m - 1 and stores nothing, a column slot
//                          past m is staged from row m - 1 and never walked.
//   tsne_zpiece_kernel     one wavefront per piece of 64 rows: lane = row adds its span sums of z in order (Z_i), the lanes' Z_i are
//                          added sequentially; tsne_seqsum_kernel adds the piece sums sequentially: Z, on the device.
//   tsne_step_kernel       one wavefront per point: the attraction over its CSR row in pieces of 64 entries, an entry per lane and the
//                          lanes' terms added in lane order; then lane d sums R_id from the span sums in order and takes the
//                          gradient-descent step of component d; writes Y, update, gains and the other copy of yf.
// and where the Kullback-Leibler divergence is asked for, tsne_kl_kernel (one wavefront per piece of 64 rows, a lane walks its CSR
// row) and tsne_seqsum_kernel again.  tsne_calibrate_kernel runs sklearn's binary search with a thread per point over its k distances.
// No atomics, no in-grid waits, no inline assembly.
#ifndef F2V_TSNE_HIP_H_
#define F2V_TSNE_HIP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f2v.h"
#include "f2v_exact.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kTsnePiece = F2V_TSNE_PIECE;                    // columns (entries, rows) per piece
constexpr uint32_t kTsneSpanCols = F2V_TSNE_PIECE * F2V_TSNE_SPAN;  // columns per span
static_assert(kTsnePiece == 64, "a piece of rows is one row per lane of a wavefront (tsne_zpiece_kernel, tsne_kl_kernel)");

// pair(i, j) of the definition: t_d = yf_id - yf_jd, a = the sum of the squares in ascending d, w = 1 / (1 + a); every operation one
// rounded fp32 operation (the library is built without contraction)
template <int D2>
__device__ __forceinline__ float tsne_pair(const float (&yi)[D2], const float (&yj)[D2], float (&t)[D2]) {
#pragma unroll
    for (int d = 0; d < D2; d++) t[d] = yi[d] - yj[d];
    float a = t[0] * t[0] + t[1] * t[1];
    if (D2 == 3) a = a + t[2] * t[2];
    return 1.0f / (1.0f + a);
}

struct TsnePairArgs {
    const float *yf;  // m x d2
    double *ws;       // [span][1 + d2][m]: a row's span sums of z, r_0 .. r_(d2-1)
    uint32_t m, spans, spans_per_slice;
};

// One piece out of LDS.  SELF: the piece may hold this lane's own row, which is skipped (w = 0 adds +0 to sums that began at +0:
// the same bits as leaving the pair out).
template <int D2, bool SELF>
__device__ __forceinline__ void tsne_piece(const float *s_y, uint32_t base, uint32_t cnt, uint32_t j0, uint32_t row, const float (&yi)[D2],
                                           float &pz, float (&pr)[D2]) {
#pragma unroll 8
    for (uint32_t q = 0; q < cnt; q++) {
        float yj[D2], t[D2];
#pragma unroll
        for (int d = 0; d < D2; d++) yj[d] = s_y[d * kTsneSpanCols + base + q];
        float w = tsne_pair<D2>(yi, yj, t);
        if (SELF) w = j0 + q == row ? 0.0f : w;
        pz = pz + w;
        const float ww = w * w;
#pragma unroll
        for (int d = 0; d < D2; d++) pr[d] = pr[d] + ww * t[d];
    }
}

// grid (ceil(m / ROWS), ceil(spans / spans_per_slice)), ROWS threads
template <int D2, int ROWS>
__global__ __launch_bounds__(ROWS) void tsne_pair_kernel(const TsnePairArgs a) {
    __shared__ __attribute__((aligned(16))) float s_y[D2 * kTsneSpanCols];
    const uint32_t m = a.m, row0 = blockIdx.x * ROWS, row = row0 + threadIdx.x, src = row < m ? row : m - 1;
    float yi[D2];
#pragma unroll
    for (int d = 0; d < D2; d++) yi[d] = a.yf[(size_t)src * D2 + d];
    const uint32_t s_begin = blockIdx.y * a.spans_per_slice;
    const uint32_t s_end = a.spans - s_begin < a.spans_per_slice ? a.spans : s_begin + a.spans_per_slice;
    for (uint32_t s = s_begin; s < s_end; s++) {  // (every bound below depends on the workgroup alone: the barriers are uniform)
        const uint32_t c0 = s * kTsneSpanCols, c1 = m - c0 < kTsneSpanCols ? m : c0 + kTsneSpanCols;
        __syncthreads();  // the span staged before has been walked
        for (uint32_t idx = threadIdx.x; idx < kTsneSpanCols; idx += ROWS) {
            const uint32_t j = c0 + idx < m ? c0 + idx : m - 1;  // a slot past the end: a valid row, never walked
#pragma unroll
            for (int d = 0; d < D2; d++) s_y[d * kTsneSpanCols + idx] = a.yf[(size_t)j * D2 + d];
        }
        __syncthreads();
        double sz = 0.0, sr[D2];
#pragma unroll
        for (int d = 0; d < D2; d++) sr[d] = 0.0;
        for (uint32_t pb = c0; pb < c1; pb += kTsnePiece) {
            const uint32_t cnt = c1 - pb < kTsnePiece ? c1 - pb : kTsnePiece;
            float pz = 0.0f, pr[D2];
#pragma unroll
            for (int d = 0; d < D2; d++) pr[d] = 0.0f;
            if (pb < row0 + ROWS && row0 < pb + cnt) tsne_piece<D2, true>(s_y, pb - c0, cnt, pb, row, yi, pz, pr);
            else tsne_piece<D2, false>(s_y, pb - c0, cnt, pb, row, yi, pz, pr);
            sz = sz + (double)pz;
#pragma unroll
            for (int d = 0; d < D2; d++) sr[d] = sr[d] + (double)pr[d];
        }
        if (row < m) {
            double *o = a.ws + (size_t)s * (1 + D2) * m + row;
            o[0] = sz;
#pragma unroll
            for (int d = 0; d < D2; d++) o[(size_t)(1 + d) * m] = sr[d];
        }
    }
}

// part[piece] = the sequential sum, from +0, of Z_i over the piece's rows; Z_i = the row's span sums of z added from +0 in span order.
// grid ceil(m / 64), 64 threads
__global__ __launch_bounds__(64) void tsne_zpiece_kernel(const double *ws, uint32_t m, uint32_t spans, uint32_t d2, double *part) {
    const uint32_t lane = threadIdx.x, row = blockIdx.x * kTsnePiece + lane;
    const uint32_t cnt = m - blockIdx.x * kTsnePiece < kTsnePiece ? m - blockIdx.x * kTsnePiece : kTsnePiece;
    double zi = 0.0;
    if (row < m)
        for (uint32_t s = 0; s < spans; s++) zi = zi + ws[(size_t)s * (1 + d2) * m + row];
    const double p = exact_lane_chain(zi, cnt);
    if (lane == 0) part[blockIdx.x] = p;
}

// *out = part[0] + part[1] + ... sequentially from +0.  One workgroup of 64 threads: the parts pass through LDS 64 at a time.
__global__ __launch_bounds__(64) void tsne_seqsum_kernel(const double *part, uint32_t count, double *out) {
    __shared__ double s_p[64];
    double sum = 0.0;
    for (uint32_t p0 = 0; p0 < count; p0 += 64) {
        const uint32_t cnt = count - p0 < 64 ? count - p0 : 64;
        __syncthreads();
        if (threadIdx.x < cnt) s_p[threadIdx.x] = part[p0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t q = 0; q < cnt; q++) sum = sum + s_p[q];
    }
    if (threadIdx.x == 0) *out = sum;
}

struct TsneStepArgs {
    const double *ws;  // the pair kernel's span sums
    const double *Z;   // the sum of tsne_seqsum_kernel
    const uint32_t *rowptr, *colids;  // P: m + 1, nnz
    const double *values;
    const float *yf_in;
    float *yf_out;
    double *y, *update, *gains;  // m x d2 each
    uint32_t m, spans;
    double ex, momentum, lr;
};

// One wavefront per point (four to a workgroup).  A piece of the point's CSR row is one entry per lane -- consecutive entries, so the
// loads coalesce -- and the lanes' terms are added sequentially in lane order: the definition's order.  Lane d then finishes component d.
template <int D2>
__global__ __launch_bounds__(256) void tsne_step_kernel(const TsneStepArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= a.m) return;  // (the whole wavefront)
    float yi[D2];
#pragma unroll
    for (int d = 0; d < D2; d++) yi[d] = a.yf_in[(size_t)i * D2 + d];
    double A[D2];
#pragma unroll
    for (int d = 0; d < D2; d++) A[d] = 0.0;
    const uint32_t e1 = a.rowptr[i + 1];
    for (uint32_t pb = a.rowptr[i]; pb < e1; pb += kTsnePiece) {
        const uint32_t cnt = e1 - pb < kTsnePiece ? e1 - pb : kTsnePiece;
        double term[D2];
#pragma unroll
        for (int d = 0; d < D2; d++) term[d] = 0.0;
        if (lane < cnt) {
            const uint32_t e = pb + lane, j = a.colids[e];
            float yj[D2], t[D2];
#pragma unroll
            for (int d = 0; d < D2; d++) yj[d] = a.yf_in[(size_t)j * D2 + d];
            const float w = tsne_pair<D2>(yi, yj, t);
            const double pw = (a.ex * a.values[e]) * (double)w;
#pragma unroll
            for (int d = 0; d < D2; d++) term[d] = pw * (double)t[d];
        }
#pragma unroll
        for (int d = 0; d < D2; d++) A[d] = A[d] + exact_lane_chain(term[d], cnt);
    }
    if (lane >= D2) return;
    const uint32_t d = lane;
    const double Ad = d == 0 ? A[0] : d == 1 ? A[1] : A[D2 - 1];
    const double Z = *a.Z;
    double R = 0.0;
    for (uint32_t s = 0; s < a.spans; s++) R = R + a.ws[((size_t)s * (1 + D2) + 1 + d) * a.m + i];
    double g = 4.0 * (Ad - R / Z);
    const size_t at = (size_t)i * D2 + d;
    double upd = a.update[at], gain = a.gains[at];
    gain = upd * g < 0.0 ? gain + 0.2 : gain * 0.8;
    gain = gain < 0.01 ? 0.01 : gain;
    g = g * gain;
    upd = a.momentum * upd - a.lr * g;
    const double y = a.y[at] + upd;
    a.gains[at] = gain;
    a.update[at] = upd;
    a.y[at] = y;
    a.yf_out[at] = (float)y;
}

struct TsneKlArgs {
    const double *Z;
    const uint32_t *rowptr, *colids;
    const double *values;
    const float *yf;
    double *part;  // one per piece of 64 rows
    uint32_t m;
};

// part[piece] = the sequential sum of the piece's row sums; a row sum = its entries in pieces of 64, each from +0, added in order.
// grid ceil(m / 64), 64 threads
template <int D2>
__global__ __launch_bounds__(64) void tsne_kl_kernel(const TsneKlArgs a) {
    const uint32_t lane = threadIdx.x, i = blockIdx.x * kTsnePiece + lane;
    const uint32_t cnt = a.m - blockIdx.x * kTsnePiece < kTsnePiece ? a.m - blockIdx.x * kTsnePiece : kTsnePiece;
    const double logZ = exact_flog(*a.Z);
    double rowsum = 0.0;
    if (i < a.m) {
        float yi[D2];
#pragma unroll
        for (int d = 0; d < D2; d++) yi[d] = a.yf[(size_t)i * D2 + d];
        const uint32_t e1 = a.rowptr[i + 1];
        for (uint32_t pb = a.rowptr[i]; pb < e1; pb += kTsnePiece) {
            const uint32_t pe = e1 - pb < kTsnePiece ? e1 : pb + kTsnePiece;
            double P = 0.0;
            for (uint32_t e = pb; e < pe; e++) {
                const uint32_t j = a.colids[e];
                float yj[D2], t[D2];
#pragma unroll
                for (int d = 0; d < D2; d++) yj[d] = a.yf[(size_t)j * D2 + d];
                const float w = tsne_pair<D2>(yi, yj, t);
                const double p = a.values[e];
                P = P + p * (exact_flog(p) - (exact_flog((double)w) - logZ));
            }
            rowsum = rowsum + P;
        }
    }
    const double s = exact_lane_chain(rowsum, cnt);
    if (lane == 0) a.part[blockIdx.x] = s;
}

// sklearn's _binary_search_perplexity in fp64, one thread per point over its k distances d_ij = -score (result order).  exp and log
// are the device library's.  cond[i][j] = p_(j|i).
__global__ __launch_bounds__(256) void tsne_calibrate_kernel(const float *scores, uint32_t m, uint32_t k, double perplexity, double *cond) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const float *sc = scores + (size_t)i * k;
    const double target = log(perplexity);
    const double inf = __builtin_huge_val();
    double beta = 1.0, lo = -inf, hi = inf, S = 0.0;
    for (uint32_t step = 0;; step++) {
        double T = 0.0;
        S = 0.0;
        for (uint32_t j = 0; j < k; j++) {
            const double d = (double)-sc[j], p = exp(-beta * d);
            S = S + p;
            T = T + d * p;
        }
        if (S == 0.0) S = 1e-8;
        const double diff = (log(S) + (beta * T) / S) - target;
        if (fabs(diff) <= 1e-5 || step == 99) break;  // the conditionals are those of the last evaluation
        if (diff > 0.0) {
            lo = beta;
            beta = hi == inf ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -inf ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    for (uint32_t j = 0; j < k; j++) cond[(size_t)i * k + j] = exp(-beta * (double)-sc[j]) / S;
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_TSNE_HIP_H_
