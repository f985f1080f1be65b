// f2v_neighbourhood.hip.h -- the neighbourhood scores of pairs on gfx950 (definition in include/f2v.h: neighbourhood scores of pairs).
//
// Integers and fp64 sums in the definition's order: the result is a function of (the CSR, the pair, kinds), whatever the launch shapes.
//   nb_degree_kernel   one wavefront per row (grid stride), lanes over the row: d(u) = |N(u)| by "differs from its predecessor, and
//                      is not u" ballots, as link_count_kernel counts it; once per handle;
//   nb_count_kernel    one thread per pair of the chunk: S, and the work items of the pair -- its pieces where there are several, else
//                      none (it then takes the direct path); the chunk's items go to a 64-bit word, one integer atomic per wavefront;
//   link_scan_*_kernel (f2v_linkpairs.hip.h) the 64-bit exclusive prefix sum of the items: the index of a pair's first item;
//   nb_fill_kernel     one thread per pair: item offset + k is (pair, piece k);
//   nb_pair_kernel     one wavefront per work item (grid stride): the items first -- they are the long ones --, then the pairs.  Lanes take
//                      64 consecutive nonzeros of S's stored row a round; a lane decides "first of its run, not u, not v", searches
//                      its id in L's stored row (a lower bound in bit-length-of-the-row steps, at most 32), and a ballot gives the
//                      round's members of W.  Every member lane forms its own Adamic-Adar and resource-allocation term (exact_flog,
//                      one division each); the terms are added to the running sums in ascending lane order, one readlane per set bit
//                      of the ballot: the definition's sequential order.  An item stores its piece's (count, sums); a pair on the
//                      direct path walks its pieces in order, adds the piece sums and stores its scores;
//   nb_finish_kernel   one thread per pair: the piece results of a pair of several pieces added in ascending piece order, and its
//                      scores; alone, without any search, where only the degree product is asked for.
// Plain launches, no in-grid waits, no float atomics; -ffp-contract=off: no fma in a term or a sum.
#ifndef F2V_NEIGHBOURHOOD_HIP_H_
#define F2V_NEIGHBOURHOOD_HIP_H_

#include "f2v.h"
#include "f2v_exact.hip.h"
#include "f2v_kernels.hip.h"
#include "f2v_linkpairs.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kNbPiece = F2V_NB_PIECE;  // nonzeros of S's stored row per piece (the definition's)
constexpr uint32_t kNbGridCap = 8192;        // workgroups of four wavefronts of nb_pair_kernel: further work items are strided over
constexpr uint32_t kNbThreadCap = 2048;      // workgroups of 256 threads of the thread-per-pair kernels: what the card holds at once

struct NbArgs {
    const uint32_t *rowptr, *colids;
    uint32_t *deg;                     // per vertex: d(u)
    const uint32_t *u, *v;             // the chunk's pairs
    uint32_t *items_of, *zero;         // per pair: its work items (0: the direct path), and the scan's second addend
    const unsigned long long *offset;  // per pair: the index of its first item
    unsigned long long *item;          // per item: pair << 32 | piece
    unsigned long long *sums;          // [0] the chunk's items
    uint32_t *piece_c;                 // per item: the piece's members of W ...
    double *piece_aa, *piece_ra;       // ... and its two sums
    double *out;                       // popcount(kinds) arrays of m, kind-major, ascending bit
    uint64_t items;                    // work items of this chunk
    uint32_t n, m, kinds;
    uint32_t spread;                   // "neighbourhood_spread": pairs of several pieces become items
};

__global__ __launch_bounds__(256) void nb_degree_kernel(const NbArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        uint32_t d = 0;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {  // (hi - q0 keeps the bound where q0 + lane would wrap)
            const bool in = lane < hi - q0;
            const uint32_t q = q0 + lane, v = in ? a.colids[q] : 0u;
            d += (uint32_t)__popcll(__ballot(in && v != u && (q == lo || a.colids[q - 1] != v)));
        }
        if (lane == 0) a.deg[u] = d;
    }
}

// S of the pair: the vertex whose stored row has fewer nonzeros, ties to the lower id
__device__ __forceinline__ bool nb_second_is_s(const NbArgs &a, uint32_t u, uint32_t v) {
    const uint32_t lu = a.rowptr[u + 1] - a.rowptr[u], lv = a.rowptr[v + 1] - a.rowptr[v];
    return lv < lu || (lv == lu && v < u);
}

__device__ __forceinline__ uint32_t nb_pieces(uint32_t len) { return len / kNbPiece + (len % kNbPiece ? 1u : 0u); }

__global__ __launch_bounds__(256) void nb_count_kernel(const NbArgs a) {
    unsigned long long items = 0;
    const uint32_t rounds = (a.m + 255u) / 256u;
    for (uint32_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const uint32_t i = r * 256u + threadIdx.x;  // (m <= 2^26: "pairs_chunk")
        if (i >= a.m) continue;
        const uint32_t u = a.u[i], v = a.v[i], s = nb_second_is_s(a, u, v) ? v : u;
        const uint32_t P = nb_pieces(a.rowptr[s + 1] - a.rowptr[s]), mine = (a.spread && P > 1) ? P : 0u;
        a.items_of[i] = mine;
        a.zero[i] = 0;
        items += mine;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) items += __shfl_xor(items, d);
    if ((threadIdx.x & 63u) == 0 && items) atomicAdd(a.sums, items);
}

__global__ __launch_bounds__(256) void nb_fill_kernel(const NbArgs a) {
    const uint32_t rounds = (a.m + 255u) / 256u;
    for (uint32_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const uint32_t i = r * 256u + threadIdx.x;
        if (i >= a.m) continue;
        const uint32_t P = a.items_of[i];
        const unsigned long long at = a.offset[i];
        for (uint32_t k = 0; k < P; k++) a.item[at + k] = ((unsigned long long)i << 32) | k;
    }
}

// One piece: the nonzeros [q0, q1) of S's stored row [slo, ...) against L's stored row [llo, lhi).  Every lane of the wavefront calls it
// with the same arguments and receives the piece's members of W and, where TERMS, its two sums, each added sequentially from +0.
template <bool TERMS>
__device__ __forceinline__ void nb_piece(const NbArgs &a, uint32_t u, uint32_t v, uint32_t slo, uint32_t q0, uint32_t q1, uint32_t llo, uint32_t lhi,
                                         uint32_t lane, uint32_t *c_out, double *aa_out, double *ra_out) {
    const uint32_t len = lhi - llo, steps = len ? 32u - (uint32_t)__builtin_clz(len) : 0u;  // a lower bound among len ids: its bit length, at most 32
    uint32_t c = 0;
    double aa = 0.0, ra = 0.0;
    for (uint32_t r0 = q0; r0 < q1; r0 += 64) {  // (wave-uniform: the bounds are the piece's)
        const bool in = lane < q1 - r0;
        const uint32_t q = r0 + lane, id = in ? a.colids[q] : 0u;
        const bool cand = in && id != u && id != v && (q == slo || a.colids[q - 1] != id);
        uint32_t lo = llo, hi = lhi;
        for (uint32_t s = 0; s < steps; s++) {
            if (cand && lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.colids[mid] < id) lo = mid + 1;
                else hi = mid;
            }
        }
        const bool hit = cand && lo < lhi && a.colids[lo] == id;
        unsigned long long mask = __ballot(hit);
        c += (uint32_t)__popcll(mask);
        if constexpr (TERMS) {
            double ta = 0.0, tr = 0.0;
            if (hit) {
                const uint32_t dw = a.deg[id];
                if (dw >= 2) ta = 1.0 / exact_flog((double)dw);
                if (dw >= 1) tr = 1.0 / (double)dw;
            }
            for (uint32_t k = 0; k < 64 && mask; k++) {  // (wave-uniform: the ballot is the same word in every lane)
                const uint32_t from = (uint32_t)__builtin_ctzll(mask);
                aa = aa + exact_readlane64(ta, from);
                ra = ra + exact_readlane64(tr, from);
                mask &= mask - 1;
            }
        }
    }
    *c_out = c;
    *aa_out = aa;
    *ra_out = ra;
}

// the scores of pair i of the chunk from |W| and the two sums
__device__ __forceinline__ void nb_emit(const NbArgs &a, uint32_t i, uint32_t u, uint32_t v, uint32_t c, double aa, double ra) {
    const uint32_t du = a.deg[u], dv = a.deg[v];
    double *o = a.out + i;
    if (a.kinds & F2V_NB_COMMON) {
        *o = (double)c;
        o += a.m;
    }
    if (a.kinds & F2V_NB_JACCARD) {
        const unsigned long long den = (unsigned long long)du + dv - c;
        *o = den ? (double)c / (double)den : 0.0;
        o += a.m;
    }
    if (a.kinds & F2V_NB_ADAMIC_ADAR) {
        *o = aa;
        o += a.m;
    }
    if (a.kinds & F2V_NB_RESOURCE) {
        *o = ra;
        o += a.m;
    }
    if (a.kinds & F2V_NB_PREFERENTIAL) *o = (double)du * (double)dv;
}

template <bool TERMS>
__global__ __launch_bounds__(256) void nb_pair_kernel(const NbArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t work = a.items + a.m;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + wave; w < work; w += (uint64_t)gridDim.x * 4) {  // (wave-uniform)
        const bool one = w < a.items;
        uint32_t i, piece = 0;
        if (one) {
            const unsigned long long it = a.item[w];
            i = (uint32_t)(it >> 32);
            piece = (uint32_t)it;
        } else {
            i = (uint32_t)(w - a.items);
            if (a.items_of[i]) continue;  // its pieces are items
        }
        const uint32_t u = a.u[i], v = a.v[i];
        const bool second = nb_second_is_s(a, u, v);
        const uint32_t s = second ? v : u, l = second ? u : v;
        const uint32_t slo = a.rowptr[s], shi = a.rowptr[s + 1], llo = a.rowptr[l], lhi = a.rowptr[l + 1];
        if (one) {
            const uint32_t q0 = slo + piece * kNbPiece, q1 = shi - q0 < kNbPiece ? shi : q0 + kNbPiece;
            uint32_t c;
            double aa, ra;
            nb_piece<TERMS>(a, u, v, slo, q0, q1, llo, lhi, lane, &c, &aa, &ra);
            if (lane == 0) {
                a.piece_c[w] = c;
                a.piece_aa[w] = aa;
                a.piece_ra[w] = ra;
            }
        } else {
            uint32_t c = 0;
            double aa = 0.0, ra = 0.0;
            for (uint32_t q0 = slo; q0 < shi; q0 += kNbPiece) {  // one piece, but under "neighbourhood_spread" = 0
                const uint32_t q1 = shi - q0 < kNbPiece ? shi : q0 + kNbPiece;
                uint32_t pc;
                double pa, pr;
                nb_piece<TERMS>(a, u, v, slo, q0, q1, llo, lhi, lane, &pc, &pa, &pr);
                c += pc;
                aa = aa + pa;
                ra = ra + pr;
                if (q1 == shi) break;  // (q0 + kNbPiece may wrap)
            }
            if (lane == 0) nb_emit(a, i, u, v, c, aa, ra);
        }
    }
}

// `every`: only the degree product is asked for -- no pair was searched, every pair is formed here
__global__ __launch_bounds__(256) void nb_finish_kernel(const NbArgs a, uint32_t every) {
    const uint32_t rounds = (a.m + 255u) / 256u;
    for (uint32_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const uint32_t i = r * 256u + threadIdx.x;
        if (i >= a.m) continue;
        uint32_t c = 0;
        double aa = 0.0, ra = 0.0;
        if (!every) {
            const uint32_t P = a.items_of[i];
            if (P == 0) continue;  // the direct path has stored its scores
            const unsigned long long at = a.offset[i];
            for (uint32_t k = 0; k < P; k++) {
                c += a.piece_c[at + k];
                aa = aa + a.piece_aa[at + k];
                ra = ra + a.piece_ra[at + k];
            }
        }
        nb_emit(a, i, a.u[i], a.v[i], c, aa, ra);
    }
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_NEIGHBOURHOOD_HIP_H_
