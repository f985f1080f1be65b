// f2v_index.hip.h -- nearest neighbours through an inverted-file index (include/f2v.h, "nearest neighbours through an index"; DESIGN
// section 20).
//
// The index is a partition of the vertices into lists (members in list order, lists + 1 offsets) and one centroid per list.  A search
// ranks the centroids per query with the exact search's own kernels (the probe order is then the defined one by construction), buckets
// the (query, probe slot) pairs by list (index_count_kernel / index_fill_kernel: integer atomics, the order inside a bucket is
// placement only) and scans every bucket against its list: index_scan_kernel.  A work item of the scan is (list, up to 32 or 128 queries
// of that list's bucket, one candidate range of the list); it scores the list's member rows, gathered as X[members[pos]], with the chains
// of nearest_kernel -- the same MFMA steps in the same de-interleaved layout for dot and cosine, the same vector-ALU chain for L2 --
// forms the keys from the ORIGINAL vertex ids and keeps the k best per (query, probe slot, range) with nearest_kernel's threshold /
// survivor buffer / rank-by-counting scheme.  Every such list is written by one work item and holds a function of its candidates
// alone; nearest_merge_kernel merges a query's probes x ranges lists, whose keys are distinct because a vertex is in one list.
#ifndef F2V_INDEX_HIP_H_
#define F2V_INDEX_HIP_H_

#include "f2v_nearest.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kIxBlock = 32;       // queries per work item of the small form: one MFMA row block
constexpr uint32_t kIxBlockBig = 128;   // ... of the large form (a bucket's full blocks; D <= 128)

struct IxItem {
    uint32_t lo, hi;    // the candidates: places [lo, hi) of the members array, inside one list
    uint32_t boff, nq;  // the queries: entries [boff, boff + nq) of the bucket array, nq <= the launch's block
    uint32_t split;     // which of the list's candidate ranges [lo, hi) is
};

struct IxArgs {
    const float *X;            // n x D, the settled matrix
    const float *Q;            // nq x D, this launch's query vectors
    const float *rq, *rc;      // cosine: 1 / |q| per query, 1 / |x| per row; nullptr otherwise
    const uint32_t *qids;      // the queries' vertex ids where a flag excludes by them; nullptr otherwise
    const uint32_t *rowptr, *colids;
    const uint32_t *members;   // the vertices in list order
    const uint32_t *bucket;    // pairs query * P + probe slot, grouped by the list they probe
    const IxItem *items;
    nn_key_t *ws;              // [query][probe slot][split][k] keys, descending; 0 = empty slot (zeroed before the launch)
    uint32_t n, D, nq, k, flags, P, splits;
    uint32_t cosine;
};

__host__ __device__ inline size_t ix_lds_bytes(uint32_t qb, uint32_t D) { return nn_lds_bytes(qb, D) + qb * sizeof(uint32_t); }

// counts[l] = the pairs that probe list l
__global__ void index_count_kernel(const uint32_t *probes, uint32_t pairs, uint32_t lists, uint32_t *counts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    const uint32_t l = probes[i];
    if (l < lists) atomicAdd(&counts[l], 1u);
}

// bucket[start[l] ..] = those pairs, in the order the atomics were served (placement only: a pair's result list is addressed by the pair)
__global__ void index_fill_kernel(const uint32_t *probes, uint32_t pairs, uint32_t lists, const uint32_t *start, uint32_t *cursor, uint32_t *bucket) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    const uint32_t l = probes[i];
    if (l < lists) bucket[start[l] + atomicAdd(&cursor[l], 1u)] = i;
}

// grid: the work items; 256 threads = WQ x (4 / WQ) wavefronts, each MI x NI tiles of 32 queries x 32 candidates, as nearest_kernel:
// <.., 1, 1, 1> takes up to 32 queries of a bucket per work item, <.., 2, 2, 2> up to 128 (D <= 128: the block lives in LDS)
template <bool L2, int WQ, int MI, int NI>
__global__ __launch_bounds__(256) void index_scan_kernel(const IxArgs a) {
    constexpr int WC = 4 / WQ;
    constexpr uint32_t QB = 32u * WQ * MI;
    static_assert(32u * WC * NI == kNnTile, "a workgroup's wavefronts cover one candidate tile");
    extern __shared__ float4 ix_smem[];
    const uint32_t nch = (a.D + kNnChunk - 1) / kNnChunk;
    float *Qs = reinterpret_cast<float *>(ix_smem);  // [chunk][query][kNnStride]
    float *Cs = Qs + (size_t)nch * QB * kNnStride;   // [candidate][kNnStride]
    nn_key_t *buf = reinterpret_cast<nn_key_t *>(Cs + kNnTile * kNnStride);
    nn_key_t *thr = buf + QB * kNnBuf;  // key of the query's k-th best so far (0: fewer than k)
    nn_key_t *scr = thr + QB;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scr + 4 * (kNnMaxK + kNnBuf));
    uint32_t *have = cnt + QB;
    uint32_t *qid = have + QB;
    float *rqs = reinterpret_cast<float *>(qid + QB);
    uint32_t *pair = reinterpret_cast<uint32_t *>(rqs + QB);  // the row's (query, probe slot) pair; kNnPadId past the item's last query

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane & 31u, h = lane >> 5;
    const uint32_t wq = wave / WC, wc = wave % WC;
    const IxItem it = a.items[blockIdx.x];

    for (uint32_t i = tid; i < QB; i += kNnThreads) {
        const bool live = i < it.nq;
        const uint32_t e = live ? a.bucket[it.boff + i] : kNnPadId, q = e / a.P;
        pair[i] = e;
        thr[i] = live ? 0 : ~0ull;  // a row past the last query accepts nothing
        cnt[i] = 0;
        have[i] = 0;
        qid[i] = a.qids && live ? a.qids[q] : kNnPadId;
        rqs[i] = a.rq && live ? a.rq[q] : 0.f;
    }
    __syncthreads();
    for (uint32_t i = tid; i < QB * nch * 8u; i += kNnThreads) {
        const uint32_t row = i / (nch * 8u), c = (i % (nch * 8u)) >> 3, c4 = i & 7u;
        const uint32_t q = pair[row] == kNnPadId ? kNnPadId : pair[row] / a.P;  // (a row past the last query is staged as zeros)
        nn_store4(Qs + ((size_t)c * QB + row) * kNnStride, c4, nn_load4(a.Q, a.nq, a.D, q, c * kNnChunk + 4 * c4));
    }
    __syncthreads();

    auto list_of = [&](uint32_t qrow) { return a.ws + ((size_t)pair[qrow] * a.splits + it.split) * a.k; };

    // nearest_kernel's compaction: one wavefront per query, always the same one; a key's place is the number of greater keys among
    // list and buffer
    auto compact = [&](bool all) {
        nn_key_t *s = scr + wave * (kNnMaxK + kNnBuf);
        for (uint32_t qrow = wave; qrow < QB; qrow += 4) {
            uint32_t cn = cnt[qrow];
            if (cn == 0 || (!all && cn < kNnBuf)) continue;
            if (cn > kNnBuf) cn = kNnBuf;
            const uint32_t ho = have[qrow], m = ho + cn;
            nn_key_t *list = list_of(qrow);
            for (uint32_t i = lane; i < ho; i += 64) s[i] = list[i];
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

    for (uint32_t cb = it.lo; cb < it.hi; cb += kNnTile) {
        nn_f32x16 acc[MI][NI];
#pragma unroll
        for (int mi = 0; mi < MI; mi++)
#pragma unroll
            for (int ni = 0; ni < NI; ni++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[mi][ni][e] = 0.f;

        // this thread stages four floats of four member rows per chunk; a place past the range is a row past the matrix: zeros
        uint32_t vrow[4];
        float4 pre[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t pos = cb + (tid >> 3) + 32u * i;
            vrow[i] = pos < it.hi ? a.members[pos] : kNnPadId;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) pre[i] = nn_load4(a.X, a.n, a.D, vrow[i], 4 * (tid & 7u));
        for (uint32_t c = 0; c < nch; c++) {
            __syncthreads();  // the previous chunk has been read
#pragma unroll
            for (int i = 0; i < 4; i++) nn_store4(Cs + ((tid >> 3) + 32u * i) * kNnStride, tid & 7u, pre[i]);
            __syncthreads();
            if (c + 1 < nch) {  // the next chunk travels while this one is multiplied
#pragma unroll
                for (int i = 0; i < 4; i++) pre[i] = nn_load4(a.X, a.n, a.D, vrow[i], (c + 1) * kNnChunk + 4 * (tid & 7u));
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

        // ---- selection: accumulator (mi, ni, e) of this lane is query row (e & 3) + 8 (e >> 2) + 4 h of its block, candidate
        // place cb + 32 (wc NI + ni) + r; keys, ties and exclusions go by the ORIGINAL vertex id found there
        uint32_t cand[NI];
        float rcv[NI];
#pragma unroll
        for (int ni = 0; ni < NI; ni++) {
            const uint32_t pos = cb + (wc * NI + ni) * 32u + r;
            cand[ni] = pos < it.hi ? a.members[pos] : kNnPadId;
            rcv[ni] = a.cosine && pos < it.hi ? a.rc[cand[ni]] : 0.f;
        }
        auto key_of = [&](int mi, int ni, int e, uint32_t qrow) {
            float s = acc[mi][ni][e];
            if constexpr (L2) s = -s;
            else if (a.cosine) s = (s * rqs[qrow]) * rcv[ni];
            return nn_make_key(s, cand[ni]);
        };
        uint32_t pend[MI][NI];
#pragma unroll
        for (int mi = 0; mi < MI; mi++)
#pragma unroll
            for (int ni = 0; ni < NI; ni++) {
                uint32_t bits = 0;
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const uint32_t qrow = (wq * MI + mi) * 32u + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (cand[ni] != kNnPadId && key_of(mi, ni, e, qrow) > thr[qrow]) bits |= 1u << e;
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
#pragma unroll
                    for (int e = 0; e < 16; e++) {
                        if (!(pend[mi][ni] & (1u << e))) continue;
                        const uint32_t qrow = (wq * MI + mi) * 32u + (e & 3) + 8 * (e >> 2) + 4 * h;
                        const nn_key_t key = key_of(mi, ni, e, qrow);
                        bool done = true;
                        if (key > thr[qrow]) {
                            const uint32_t v = qid[qrow];
                            const bool out = ((a.flags & 1u) && cand[ni] == v) || ((a.flags & 2u) && nn_is_neighbour(a.rowptr, a.colids, v, cand[ni]));
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
    for (uint32_t qrow = wave; qrow < it.nq; qrow += 4) {
        nn_key_t *list = list_of(qrow);
        for (uint32_t i = have[qrow] + lane; i < a.k; i += 64) list[i] = 0;
    }
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_INDEX_HIP_H_
