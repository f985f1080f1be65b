// f2v_nearest.hip.h -- nearest-neighbour queries over the embedding matrix (include/f2v.h, "nearest neighbours").
//
// One launch of nearest_kernel scores a block of queries (QB = 32 or 128, resident in LDS) against one candidate range of the
// matrix (a "split") in tiles of 128 candidates and keeps, per query, the k best candidates of that range; nearest_merge_kernel
// combines the splits.  Scores are the fp32 fmaf chains of f2v.h:
//   dot / cosine: v_mfma_f32_32x32x2_f32 -- A = 32 queries, B = 32 candidates, lane half h feeds dimension 2s + h at step s, so the
//     accumulator is the chain over ascending d bit for bit; cosine multiplies the two reciprocal norms in behind it;
//   L2: the vector ALU in the accumulator layout of that MFMA (lane = candidate, register = query), one subtraction and one fma
//     per pair and dimension.
// Selection works on 64-bit keys (order-preserving image of the score in the high word, ~id in the low word), so "score descending,
// ties by ascending id, NaN last" is plain unsigned order and every key of a query is distinct: ranks are found by counting greater
// keys, with no float atomics, and what a query's list holds cannot depend on the order in which survivors arrived.
#ifndef F2V_NEAREST_HIP_H_
#define F2V_NEAREST_HIP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kNnChunk = 32;    // dimensions staged per step of the k loop
constexpr uint32_t kNnStride = 36;   // floats per staged row: 16 even dimensions, 16 odd ones, 4 of padding (ds_read_b128 without bank conflicts)
constexpr uint32_t kNnTile = 128;    // candidates per tile
constexpr uint32_t kNnBuf = 32;      // survivor slots per query between two compactions
constexpr uint32_t kNnMaxK = 128;    // F2V_NEAREST_MAX_K
constexpr uint32_t kNnThreads = 256;
constexpr uint32_t kNnPadId = 0xFFFFFFFFu;

typedef float nn_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long nn_key_t;

struct NnArgs {
    const float *X;            // n x D, the settled matrix
    const float *Q;            // nq x D, this launch's query vectors
    const float *rq, *rc;      // cosine: 1 / |q| per query, 1 / |x| per row; nullptr otherwise
    const uint32_t *qids;      // the queries' vertex ids where a flag excludes by them; nullptr otherwise
    const uint32_t *rowptr, *colids;
    nn_key_t *ws;              // [query][split][k] keys, descending; 0 = empty slot
    uint32_t n, D, nq, k, flags, splits, tiles_per_split;
    uint32_t cosine;
};

// score descending, id ascending, NaN below every number  ==  key descending
__device__ inline nn_key_t nn_make_key(float s, uint32_t id) {
    if (s != s) return (nn_key_t)(uint32_t)~id;
    uint32_t u = __float_as_uint(s + 0.0f);  // -0 and +0 are one score
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((nn_key_t)u << 32) | (uint32_t)~id;
}

__device__ inline void nn_wave_sync() {  // LDS traffic of one wavefront is served in order: only the compiler has to be told
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline bool nn_is_neighbour(const uint32_t *rowptr, const uint32_t *colids, uint32_t v, uint32_t cand) {
    uint32_t lo = rowptr[v], hi = rowptr[v + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t c = colids[mid];
        if (c == cand) return true;
        if (c < cand) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

__host__ __device__ inline size_t nn_lds_bytes(uint32_t qb, uint32_t D) {
    const size_t nch = (D + kNnChunk - 1) / kNnChunk;
    return (nch * qb * kNnStride + (size_t)kNnTile * kNnStride) * sizeof(float) +
           ((size_t)qb * kNnBuf + qb + 4 * (kNnMaxK + kNnBuf)) * sizeof(nn_key_t) + (size_t)4 * qb * sizeof(uint32_t);
}

// four floats of row `row` of M (rows x D) from dimension d on; zeros past the row's end and past the last row
__device__ inline float4 nn_load4(const float *M, uint32_t rows, uint32_t D, uint32_t row, uint32_t d) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows && d < D) {
        const float *p = M + (size_t)row * D + d;
        if ((D & 3u) == 0) {
            v = *reinterpret_cast<const float4 *>(p);
        } else {
            v.x = p[0];
            if (d + 1 < D) v.y = p[1];
            if (d + 2 < D) v.z = p[2];
            if (d + 3 < D) v.w = p[3];
        }
    }
    return v;
}

// ... stored as two even and two odd dimensions of a staged row (`c4`: which four of the chunk's 32)
__device__ inline void nn_store4(float *row, uint32_t c4, float4 v) {
    *reinterpret_cast<float2 *>(row + 2 * c4) = make_float2(v.x, v.z);
    *reinterpret_cast<float2 *>(row + 16 + 2 * c4) = make_float2(v.y, v.w);
}

// grid (query blocks, splits), 256 threads = WQ x (4 / WQ) wavefronts, each MI x NI tiles of 32 queries x 32 candidates
template <bool L2, int WQ, int MI, int NI>
__global__ __launch_bounds__(256) void nearest_kernel(const NnArgs a) {
    constexpr int WC = 4 / WQ;
    constexpr uint32_t QB = 32u * WQ * MI;
    static_assert(32u * WC * NI == kNnTile, "a workgroup's wavefronts cover one candidate tile");
    extern __shared__ float4 nn_smem[];
    const uint32_t nch = (a.D + kNnChunk - 1) / kNnChunk;
    float *Qs = reinterpret_cast<float *>(nn_smem);  // [chunk][query][kNnStride]
    float *Cs = Qs + (size_t)nch * QB * kNnStride;   // [candidate][kNnStride]
    nn_key_t *buf = reinterpret_cast<nn_key_t *>(Cs + kNnTile * kNnStride);
    nn_key_t *thr = buf + QB * kNnBuf;  // key of the query's k-th best so far (0: fewer than k)
    nn_key_t *scr = thr + QB;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scr + 4 * (kNnMaxK + kNnBuf));
    uint32_t *have = cnt + QB;
    uint32_t *qid = have + QB;
    float *rqs = reinterpret_cast<float *>(qid + QB);

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t wq = wave / WC, wc = wave % WC;
    const uint32_t q0 = blockIdx.x * QB, split = blockIdx.y;
    const uint32_t tiles = (a.n + kNnTile - 1) / kNnTile;
    const uint32_t tile_lo = split * a.tiles_per_split;
    const uint32_t tile_hi = tile_lo + a.tiles_per_split < tiles ? tile_lo + a.tiles_per_split : tiles;

    for (uint32_t i = tid; i < QB; i += kNnThreads) {
        const bool live = q0 + i < a.nq;
        thr[i] = live ? 0 : ~0ull;  // a row past the last query accepts nothing (cheaper than testing the row per accumulator)
        cnt[i] = 0;
        have[i] = 0;
        qid[i] = a.qids && live ? a.qids[q0 + i] : kNnPadId;
        rqs[i] = a.rq && live ? a.rq[q0 + i] : 0.f;
    }
    for (uint32_t i = tid; i < QB * nch * 8u; i += kNnThreads) {
        const uint32_t row = i / (nch * 8u), c = (i % (nch * 8u)) >> 3, c4 = i & 7u;
        nn_store4(Qs + ((size_t)c * QB + row) * kNnStride, c4, nn_load4(a.Q, a.nq, a.D, q0 + row, c * kNnChunk + 4 * c4));
    }
    __syncthreads();

    auto list_of = [&](uint32_t qrow) { return a.ws + ((size_t)(q0 + qrow) * a.splits + split) * a.k; };

    // Fold the survivor buffers into the queries' sorted lists (all of them, or the full ones only).  One wavefront per query,
    // always the same one; a key's place is the number of greater keys among list and buffer.
    auto compact = [&](bool all) {
        nn_key_t *s = scr + wave * (kNnMaxK + kNnBuf);
        for (uint32_t qrow = wave; qrow < QB; qrow += 4) {
            uint32_t cn = cnt[qrow];
            if (cn == 0 || (!all && cn < kNnBuf)) continue;
            if (cn > kNnBuf) cn = kNnBuf;
            const uint32_t ho = have[qrow], m = ho + cn;
            nn_key_t *list = list_of(qrow);
            for (uint32_t i = lane; i < ho; i += 64) s[i] = list[i];  // (a list belongs to this one wavefront until the kernel ends: plain accesses, ordered by nn_wave_sync)
            if (lane < cn) s[ho + lane] = buf[qrow * kNnBuf + lane];
            nn_wave_sync();
            for (uint32_t e = lane; e < m; e += 64) {
                const nn_key_t key = s[e];
                uint32_t rank = 0;
                for (uint32_t i = 0; i < m; i++) rank += s[i] > key ? 1u : 0u;
                if (rank < a.k) list[rank] = key;
                if (rank == a.k - 1) thr[qrow] = key;
            }
            nn_wave_sync();
            if (lane == 0) {
                have[qrow] = m < a.k ? m : a.k;
                cnt[qrow] = 0;
            }
            nn_wave_sync();
        }
    };

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

        // ---- selection: accumulator (mi, ni, e) of this lane is query row (e & 3) + 8 (e >> 2) + 4 h, candidate column r
        float rcv[NI];
#pragma unroll
        for (int ni = 0; ni < NI; ni++) {
            const uint32_t cand = cb + (wc * NI + ni) * 32u + r;
            rcv[ni] = a.cosine && cand < a.n ? a.rc[cand] : 0.f;
        }
        auto key_of = [&](int mi, int ni, int e, uint32_t qrow, uint32_t cand) {
            float s = acc[mi][ni][e];
            if constexpr (L2) s = -s;
            else if (a.cosine) s = (s * rqs[qrow]) * rcv[ni];
            return nn_make_key(s, cand);
        };
        uint32_t pend[MI][NI];
#pragma unroll
        for (int mi = 0; mi < MI; mi++)
#pragma unroll
            for (int ni = 0; ni < NI; ni++) {
                const uint32_t cand = cb + (wc * NI + ni) * 32u + r;
                uint32_t bits = 0;
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const uint32_t qrow = (wq * MI + mi) * 32u + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (cand < a.n && key_of(mi, ni, e, qrow, cand) > thr[qrow]) bits |= 1u << e;
                }
                pend[mi][ni] = bits;
            }
        for (;;) {
            bool stuck = false;
#pragma unroll
            for (int mi = 0; mi < MI; mi++)
#pragma unroll
                for (int ni = 0; ni < NI; ni++) {
                    if (!pend[mi][ni]) continue;
                    const uint32_t cand = cb + (wc * NI + ni) * 32u + r;
#pragma unroll
                    for (int e = 0; e < 16; e++) {
                        if (!(pend[mi][ni] & (1u << e))) continue;
                        const uint32_t qrow = (wq * MI + mi) * 32u + (e & 3) + 8 * (e >> 2) + 4 * h;
                        const nn_key_t key = key_of(mi, ni, e, qrow, cand);
                        bool done = true;
                        if (key > thr[qrow]) {
                            const uint32_t v = qid[qrow];
                            const bool out = ((a.flags & 1u) && cand == v) || ((a.flags & 2u) && nn_is_neighbour(a.rowptr, a.colids, v, cand));
                            if (!out) {
                                const uint32_t slot = atomicAdd(&cnt[qrow], 1u);
                                if (slot < kNnBuf) buf[qrow * kNnBuf + slot] = key;
                                else done = false;
                            }
                        }
                        if (done) pend[mi][ni] &= ~(1u << e);
                        else stuck = true;
                    }
                }
            if (!__syncthreads_or(stuck ? 1 : 0)) break;
            compact(false);
            __syncthreads();
        }
    }

    __syncthreads();
    compact(true);
    for (uint32_t qrow = wave; qrow < QB; qrow += 4) {
        if (q0 + qrow >= a.nq) continue;
        nn_key_t *list = list_of(qrow);
        for (uint32_t i = have[qrow] + lane; i < a.k; i += 64) list[i] = 0;
    }
}

// One workgroup per query: the k greatest of its splits' sorted lists, decoded.  A key's rank is the sum, over the lists, of the
// keys greater than it (binary search); keys are distinct, empty slots (0) are skipped.
__global__ __launch_bounds__(256) void nearest_merge_kernel(const nn_key_t *ws, uint32_t splits, uint32_t k, uint32_t *ids_out, float *scores_out) {
    const uint32_t q = blockIdx.x, m = splits * k;
    const nn_key_t *L = ws + (size_t)q * m;
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
        ids_out[(size_t)q * k + i] = kNnPadId;
        scores_out[(size_t)q * k + i] = -__builtin_inff();
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < m; e += blockDim.x) {
        const nn_key_t key = L[e];
        if (key == 0) continue;
        uint32_t rank = 0;
        for (uint32_t l = 0; l < splits && rank < k; l++) {
            const nn_key_t *P = L + (size_t)l * k;
            uint32_t lo = 0, hi = k;  // first slot whose key is not greater
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (P[mid] > key) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank >= k) continue;
        const uint32_t u = (uint32_t)(key >> 32);
        ids_out[(size_t)q * k + rank] = ~(uint32_t)key;
        scores_out[(size_t)q * k + rank] = u == 0 ? __builtin_nanf("") : __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
    }
}

// out[i] = row ids[i] of X
__global__ void nearest_gather_kernel(const float *X, const uint32_t *ids, uint32_t nq, uint32_t D, float *out) {
    const size_t total = (size_t)nq * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        out[i] = X[(size_t)ids[i / D] * D + i % D];
}

// out[v] = 1 / sqrt(chain_d fma(x_d, x_d, acc)), 0 for a zero row (square root and division correctly rounded)
__global__ void nearest_rnorm_kernel(const float *M, uint32_t rows, uint32_t D, float *out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= rows) return;
    const float *p = M + (size_t)v * D;
    float acc = 0.f;
    if ((D & 3u) == 0) {
        for (uint32_t d = 0; d < D; d += 4) {
            const float4 x = *reinterpret_cast<const float4 *>(p + d);
            acc = __builtin_fmaf(x.x, x.x, acc);
            acc = __builtin_fmaf(x.y, x.y, acc);
            acc = __builtin_fmaf(x.z, x.z, acc);
            acc = __builtin_fmaf(x.w, x.w, acc);
        }
    } else {
        for (uint32_t d = 0; d < D; d++) acc = __builtin_fmaf(p[d], p[d], acc);
    }
    out[v] = acc == 0.f ? 0.f : 1.0f / __builtin_sqrtf(acc);  // hipcc's default: both correctly rounded (no fast-math, no native_*)
}

// counts[0] += |top-k(v) n N(v)|, counts[1] += min(k, distinct neighbours of v other than v), one thread per query
__global__ void nearest_recall_kernel(const uint32_t *ids, const uint32_t *qids, uint32_t nq, uint32_t k, const uint32_t *rowptr,
                                      const uint32_t *colids, unsigned long long *counts) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint32_t v = qids[q];
    uint32_t hits = 0, possible = 0;
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t id = ids[(size_t)q * k + i];
        if (id != kNnPadId && nn_is_neighbour(rowptr, colids, v, id)) hits++;
    }
    for (uint32_t p = rowptr[v]; p < rowptr[v + 1] && possible < k; p++) {
        const uint32_t c = colids[p];
        if (c != v && (p == rowptr[v] || colids[p - 1] != c)) possible++;
    }
    atomicAdd(counts, (unsigned long long)hits);
    atomicAdd(counts + 1, (unsigned long long)possible);
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_NEAREST_HIP_H_
