// f2v_louvain.hip.h -- the communities of the graph (Louvain) and the agreement of two labellings on gfx950 (definitions in
// include/f2v.h: communities).
//
// Integers only until the final Q: every result is a function of (CSR, seed, max_levels, max_sweeps), whatever the launch shapes.
//   louvain_symmetry_kernel  16 lanes per row: every nonzero (u, v), u != v, is looked up in row v (binary search);
//   louvain_degree_kernel    16 lanes per row of the CSR: k(u) = distinct neighbours other than u + 2 loop(u), and 2m;
//   louvain_bin_kernel       placement: a unit -- a node when moving, a community when aggregating -- goes to the list of its
//                            (class, form); once counting, once filling, tallied per workgroup in LDS first.  The order inside a list
//                            is that of arrival: placement only;
//   louvain_gather_kernel    <FORM, AGG>: the weights from a unit to the communities around it are summed in an open-addressing table
//                            of (community, weight): integer compare-and-swap on the keys, integer adds on the weights, every probe loop
//                            bounded by the table's slots, a table at least twice as long as the unit's row(s).
//                            FORM 0: 16 lanes per unit, 16 units per workgroup, tables of one size in LDS;
//                            FORM 1: a workgroup per unit, its table in LDS;  FORM 2: a workgroup of 1024 lanes per unit, its table in
//                            the workspace.
//                            AGG = false (a sub-round's decisions): the score and the tie rule over the table, the decision to next[i];
//                            AGG = true (a coarse row): the table's entries are the row, the entry of the community itself its loop;
//   louvain_apply_kernel     the sub-round's moves: labels, tot and size by integer atomics, the moves counted once per wavefront;
//   louvain_qnum_kernel      the weight inside communities and the sum of tot^2: two 64-bit integer sums, 16 lanes per row; the rows of
//                            the third form are left to louvain_qnum_wide_kernel, a workgroup each;
//   louvain_flag / _scan_* / _member_* / _relabel kernels  the renumbering (present flags, exclusive prefix sums), the members grouped
//                            by community, the vertices' labels;
//   agree_count_kernel, agree_piece_kernel, agree_log_kernel  the contingency table by integer atomics, then n flog(n) over pieces
//                            of 1024 consecutive cells, each piece summed in order by one lane.
// Plain launches on the handle's stream, no in-grid waits, no float atomics.
#ifndef F2V_LOUVAIN_HIP_H_
#define F2V_LOUVAIN_HIP_H_

#include "f2v.h"
#include "f2v_kernels.hip.h"
#include "f2v_nearest.hip.h"
#include "f2v_exact.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kLouvainShortLimit = 256;   // the largest "louvain_short_max": 16 tables of 512 slots are 64 KiB of LDS
constexpr uint32_t kLouvainLdsLimit = 8192;    // the largest "louvain_lds_slots": 64 KiB of keys and weights
constexpr uint32_t kLouvainHeader = 96;        // LDS words in front of the tables: 16 cursors, 4 words per wavefront of the workgroup's reduction
constexpr uint32_t kLouvainWideThreads = 1024; // lanes of a workgroup whose table lies in the workspace: its unit's row is one chain of dependent atomics however wide it is
constexpr uint32_t kLouvainEmpty = 0xFFFFFFFFu;  // no key (ids are below n <= 2^32 - 1)
constexpr uint32_t kLouvainScanTile = 1024;
constexpr uint32_t kLouvainBins = F2V_LOUVAIN_PHASES * 3;
constexpr uint32_t kAgreePiece = 1024;

// slots of the table of a unit whose rows hold `len` nonzeros: a power of two, at least 2 len (and at least 2)
__host__ __device__ inline uint32_t louvain_slots(uint32_t len) {
    uint32_t s = 2;
    while (s < 2 * (uint64_t)len && s < 0x80000000u) s <<= 1;
    return s;
}

struct LouvainArgs {
    // the level's graph: row i is cols[rowbeg[i] .. rowend[i]) with weights wts (NULL: 1 each); level 0 is the CSR itself, where a
    // column equal to its predecessor is skipped (`dedupe`); a column equal to its row is skipped at every level
    const uint32_t *rowbeg, *rowend, *cols, *wts;
    const uint32_t *k, *loop;        // per node
    uint32_t *c, *next, *tot, *size; // per node / community
    const uint32_t *key;             // gather: the community of a node (c, or the renumbered kept community when aggregating)
    uint32_t *units;                 // gather: this launch's units
    unsigned long long *table_at;    // FORM 2: per unit of this launch the first word of its table
    uint32_t *table;
    uint32_t *mstart, *members;          // aggregation: the nodes of community C are members[mstart[C] .. mstart[C + 1])
    uint32_t *orowbeg, *orowend, *ocols, *owts, *oloop, *ok;  // aggregation: the next level's graph
    uint32_t *kept, *newid, *ccount, *vlabel;
    unsigned long long *sums;        // [0] moves, [1] inside weight, [2] sum of tot^2, [3] 2m
    unsigned long long *bins;        // [0..23] units per (class, form), [24..31] table words per class, [32..63] the fill's cursors
    uint32_t start[kLouvainBins];    // louvain_bin_kernel<true>: the first place of every list
    uint64_t level_mix;              // mix64(seed + level)
    uint32_t N, n, count, slots, dedupe, agg, two_m, short_max, lds_slots;
    uint32_t K;                      // aggregation: the next level's nodes (a coarse row's table holds at most K keys)
};

// what sizes a unit's table and decides its form: the nonzeros of its rows, for a community no more than the K keys there are
__device__ __forceinline__ uint32_t louvain_unit_len(const LouvainArgs &a, bool agg, uint32_t unit) {
    if (!agg) return a.rowend[unit] - a.rowbeg[unit];
    const uint32_t len = a.orowbeg[unit + 1] - a.orowbeg[unit];
    return len < a.K ? len : a.K;
}

__device__ __forceinline__ uint32_t louvain_class(const LouvainArgs &a, uint32_t i) { return (uint32_t)(mix64(a.level_mix ^ (uint64_t)i) % F2V_LOUVAIN_PHASES); }

// ---- prepare ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void louvain_symmetry_kernel(const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint32_t *bad) {
    const uint32_t l = threadIdx.x & 15u;
    for (uint64_t u = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4); u < n; u += (uint64_t)gridDim.x * 16) {
        const uint32_t lo = rowptr[u], hi = rowptr[u + 1];
        for (uint32_t q = lo + l; q < hi; q += 16) {
            const uint32_t v = colids[q];
            if (v != (uint32_t)u && !(v < n && nn_is_neighbour(rowptr, colids, v, (uint32_t)u))) *bad = 1u;
        }
    }
}

__global__ __launch_bounds__(256) void louvain_degree_kernel(const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint32_t *k, uint32_t *loop,
                                                             unsigned long long *sums) {
    const uint32_t l = threadIdx.x & 15u;
    unsigned long long mine = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4); u < n; u += (uint64_t)gridDim.x * 16) {
        const uint32_t lo = rowptr[u], hi = rowptr[u + 1];
        uint32_t deg = 0, self = 0;
        for (uint32_t q = lo + l; q < hi; q += 16) {
            const uint32_t v = colids[q];
            if (q > lo && colids[q - 1] == v) continue;
            if (v == (uint32_t)u) self = 1;
            else deg++;
        }
#pragma unroll
        for (uint32_t d = 8; d; d >>= 1) {
            deg += __shfl_xor(deg, d);
            self |= __shfl_xor(self, d);
        }
        if (l == 0) {
            k[u] = deg + 2 * self;
            loop[u] = self;
            mine += deg + 2 * self;
        }
    }
    if (mine) atomicAdd(sums + 3, mine);
}

__global__ __launch_bounds__(256) void louvain_init_kernel(const LouvainArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    a.c[i] = (uint32_t)i;
    a.next[i] = (uint32_t)i;
    a.kept[i] = (uint32_t)i;
    a.tot[i] = a.k[i];
    a.size[i] = 1u;
}

// ---- placement -------------------------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void louvain_bin_kernel(const LouvainArgs a) {
    __shared__ unsigned long long tally[32], base[32];  // the workgroup's units per list and table words per class; their first places
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < 32) tally[threadIdx.x] = 0;
    __syncthreads();
    uint32_t len = 0, cls = 0, slots = 0, form = 0, bin = 0;
    bool listed = i < a.count;
    if (listed) {
        len = louvain_unit_len(a, a.agg != 0, (uint32_t)i);
        listed = a.agg || len != 0;  // a node without a nonzero decides nothing
        cls = a.agg ? 0u : louvain_class(a, (uint32_t)i);
        slots = louvain_slots(len);
        form = len <= a.short_max ? 0u : slots <= a.lds_slots ? 1u : 2u;
        bin = cls * 3 + form;
    }
    unsigned long long rank = 0, word = 0;
    if (listed) {
        rank = atomicAdd(&tally[bin], 1ull);
        if (form == 2) word = atomicAdd(&tally[kLouvainBins + cls], 2ull * slots);
    }
    __syncthreads();
    if (threadIdx.x < 32 && tally[threadIdx.x]) base[threadIdx.x] = atomicAdd(a.bins + (FILL ? 32 : 0) + threadIdx.x, tally[threadIdx.x]);
    if (!FILL) return;
    __syncthreads();
    if (listed) {
        const uint32_t at = a.start[bin] + (uint32_t)(base[bin] + rank);
        a.units[at] = (uint32_t)i;
        if (form == 2) a.table_at[at] = base[kLouvainBins + cls] + word;
    }
}

// ---- the table -------------------------------------------------------------------------------------------------------------------
struct LouvainBest {
    long long score;
    uint32_t id, ea;
};

__device__ __forceinline__ void louvain_take(LouvainBest &x, long long score, uint32_t id) {
    if (id != kLouvainEmpty && (x.id == kLouvainEmpty || score > x.score || (score == x.score && id < x.id))) {
        x.score = score;
        x.id = id;
    }
}

template <uint32_t W>
__device__ __forceinline__ void louvain_lanes_best(LouvainBest &x) {
#pragma unroll
    for (uint32_t d = W / 2; d; d >>= 1) {
        const long long score = __shfl_xor(x.score, d);
        const uint32_t id = __shfl_xor(x.id, d), ea = __shfl_xor(x.ea, d);
        louvain_take(x, score, id);
        x.ea += ea;  // (one slot at most holds the node's own community)
    }
}

template <int FORM>
__device__ __forceinline__ void louvain_sync() {
    if constexpr (FORM == 0) nn_wave_sync();
    else {
        if constexpr (FORM == 2) __threadfence();
        __syncthreads();
    }
}

template <int FORM>
__device__ __forceinline__ uint32_t louvain_load(const uint32_t *p) {
    if constexpr (FORM == 2) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

template <int FORM, bool AGG>
__global__ __launch_bounds__(FORM == 2 ? kLouvainWideThreads : 256) void louvain_gather_kernel(const LouvainArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t louvain_smem[];
    constexpr uint32_t kThreads = FORM == 2 ? kLouvainWideThreads : 256u, G = FORM == 0 ? 16u : kThreads, kGroups = kThreads / G;
    constexpr uint32_t SUB = AGG ? 16u : G;  // lanes over one member's row
    const uint32_t tid = threadIdx.x, t = tid % G, grp = tid / G;
    uint32_t *cursor = louvain_smem + grp, *scratch = louvain_smem + 16;
    for (uint64_t w0 = (uint64_t)blockIdx.x * kGroups; w0 < a.count; w0 += (uint64_t)gridDim.x * kGroups) {
        const bool active = w0 + grp < a.count;
        uint32_t unit = 0, slots = 2, *keys = louvain_smem + kLouvainHeader;
        if (active) {
            unit = a.units[w0 + grp];
            const uint32_t len = louvain_unit_len(a, AGG, unit);
            slots = FORM == 0 ? a.slots : louvain_slots(len);
            if (FORM == 0) keys += (size_t)grp * 2 * slots;
            if (FORM == 2) keys = a.table + a.table_at[w0 + grp];
        }
        uint32_t *wts = keys + slots;
        const uint32_t mask = slots - 1u, shift = 32u - (uint32_t)__builtin_ctz(slots);
        if (active) {
            for (uint32_t s = t; s < slots; s += G) {
                if (FORM == 2) {
                    __hip_atomic_store(&keys[s], kLouvainEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&wts[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else {
                    keys[s] = kLouvainEmpty;
                    wts[s] = 0u;
                }
            }
            if (t == 0) *cursor = 0u;
        }
        louvain_sync<FORM>();
        if (active) {
            const uint32_t m0 = AGG ? a.mstart[unit] : 0u, m1 = AGG ? a.mstart[unit + 1] : 1u;
            for (uint32_t m = m0 + t / SUB; m < m1; m += G / SUB) {
                const uint32_t i = AGG ? a.members[m] : unit, lo = a.rowbeg[i], hi = a.rowend[i];
                for (uint32_t q = lo + t % SUB; q < hi; q += SUB) {
                    const uint32_t j = a.cols[q];
                    if (j == i || (a.dedupe && q > lo && a.cols[q - 1] == j)) continue;
                    const uint32_t d = a.key[j], w = a.wts ? a.wts[q] : 1u;
                    uint32_t s = (d * 0x9E3779B1u) >> shift;
                    for (uint32_t probe = 0; probe < slots; probe++) {  // (the table is at most half full: a free slot comes first)
                        const uint32_t old = atomicCAS(&keys[s], kLouvainEmpty, d);
                        if (old == kLouvainEmpty || old == d) {
                            atomicAdd(&wts[s], w);
                            break;
                        }
                        s = (s + 1u) & mask;
                    }
                }
            }
        }
        louvain_sync<FORM>();
        if constexpr (!AGG) {
            LouvainBest x{0, kLouvainEmpty, 0u};
            uint32_t own = 0, ki = 0;
            if (active) {
                own = a.key[unit];
                ki = a.k[unit];
                for (uint32_t s = t; s < slots; s += G) {
                    const uint32_t d = louvain_load<FORM>(&keys[s]);
                    if (d == kLouvainEmpty) continue;
                    const uint32_t e = louvain_load<FORM>(&wts[s]), tot = a.tot[d] - (d == own ? ki : 0u);
                    louvain_take(x, (long long)e * (long long)a.two_m - (long long)ki * (long long)tot, d);
                    if (d == own) x.ea = e;
                }
            }
            if constexpr (FORM == 0) louvain_lanes_best<16>(x);
            else {
                louvain_lanes_best<64>(x);
                if ((tid & 63u) == 0) {
                    uint32_t *o = scratch + 4 * (tid >> 6);
                    o[0] = (uint32_t)(unsigned long long)x.score;
                    o[1] = (uint32_t)((unsigned long long)x.score >> 32);
                    o[2] = x.id;
                    o[3] = x.ea;
                }
                __syncthreads();
                if (tid == 0)
                    for (uint32_t wv = 1; wv < kThreads / 64; wv++) {
                        const uint32_t *o = scratch + 4 * wv;
                        louvain_take(x, (long long)(((unsigned long long)o[1] << 32) | o[0]), o[2]);
                        x.ea += o[3];
                    }
            }
            if (active && t == 0) {
                uint32_t to = own;
                if (x.id != kLouvainEmpty && x.id != own) {
                    const long long stay = (long long)x.ea * (long long)a.two_m - (long long)ki * (long long)(a.tot[own] - ki);
                    const bool swap = a.size[own] == 1u && a.size[x.id] == 1u && x.id > own;  // two singletons never swap
                    if (x.score > stay && !swap) to = x.id;
                }
                a.next[unit] = to;
            }
        } else {
            uint32_t base = 0;
            if (active) {
                base = a.orowbeg[unit];
                for (uint32_t s = t; s < slots; s += G) {
                    const uint32_t d = louvain_load<FORM>(&keys[s]);
                    if (d == kLouvainEmpty) continue;
                    const uint32_t e = louvain_load<FORM>(&wts[s]);
                    if (d == unit) a.oloop[unit] += e / 2u;  // (ordered pairs inside: every edge twice; one slot, one lane)
                    else {
                        const uint32_t at = base + atomicAdd(cursor, 1u);
                        a.ocols[at] = d;
                        a.owts[at] = e;
                    }
                }
            }
            louvain_sync<FORM == 0 ? 0 : 1>();
            if (active && t == 0) a.orowend[unit] = base + *cursor;
        }
        louvain_sync<FORM == 0 ? 0 : 1>();  // (the header and the table are reused by the next unit)
    }
}

// ---- a sub-round's moves, a sweep's Qnum ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void louvain_apply_kernel(const LouvainArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (i < a.N) {
        const uint32_t from = a.c[i], to = a.next[i];
        if (from != to) {
            moved = true;
            const uint32_t ki = a.k[i];
            atomicSub(&a.tot[from], ki);
            atomicAdd(&a.tot[to], ki);
            atomicSub(&a.size[from], 1u);
            atomicAdd(&a.size[to], 1u);
            a.c[i] = to;
        }
    }
    const unsigned long long mask = __ballot(moved);
    if (mask && (threadIdx.x & 63u) == 0) atomicAdd(a.sums + 0, (unsigned long long)__popcll(mask));
}

__global__ __launch_bounds__(256) void louvain_qnum_kernel(const LouvainArgs a) {
    const uint32_t l = threadIdx.x & 15u;
    unsigned long long inside = 0, squares = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < a.N; i += (uint64_t)gridDim.x * 16) {
        const uint32_t lo = a.rowbeg[i], hi = a.rowend[i], ci = a.c[i];
        const bool wide = hi - lo > a.short_max && louvain_slots(hi - lo) > a.lds_slots;  // a row of louvain_qnum_wide_kernel (the placement's third form)
        for (uint32_t q = lo + l; q < hi && !wide; q += 16) {
            const uint32_t j = a.cols[q];
            if (j == (uint32_t)i || (a.dedupe && q > lo && a.cols[q - 1] == j)) continue;
            if (a.c[j] == ci) inside += a.wts ? a.wts[q] : 1u;
        }
        if (l == 0) {
            const unsigned long long tot = a.tot[i];
            inside += 2ull * a.loop[i];
            squares += tot * tot;
        }
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        inside += __shfl_xor(inside, d);
        squares += __shfl_xor(squares, d);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (inside) atomicAdd(a.sums + 1, inside);
        if (squares) atomicAdd(a.sums + 2, squares);
    }
}

// the inside weight of the rows that louvain_qnum_kernel leaves out: a workgroup per row of one class's third list
__global__ __launch_bounds__(256) void louvain_qnum_wide_kernel(const LouvainArgs a) {
    unsigned long long inside = 0;
    for (uint32_t w = blockIdx.x; w < a.count; w += gridDim.x) {
        const uint32_t i = a.units[w], lo = a.rowbeg[i], hi = a.rowend[i], ci = a.c[i];
        for (uint32_t q = lo + threadIdx.x; q < hi; q += 256) {
            const uint32_t j = a.cols[q];
            if (j == i || (a.dedupe && q > lo && a.cols[q - 1] == j)) continue;
            if (a.c[j] == ci) inside += a.wts ? a.wts[q] : 1u;
        }
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) inside += __shfl_xor(inside, d);
    if ((threadIdx.x & 63u) == 0 && inside) atomicAdd(a.sums + 1, inside);
}

// ---- aggregation -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void louvain_flag_kernel(const LouvainArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.N) a.newid[a.kept[i]] = 1u;
}

// exclusive prefix sums of x[0 .. count) in place, the total to x[count]: tile sums, one workgroup over them, the tiles again
__device__ __forceinline__ uint32_t louvain_block_scan(uint32_t x, uint32_t *s, uint32_t *sum) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    s[t] = x;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t y = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    *sum = s[255];
    return s[t] - x;
}

__device__ __forceinline__ uint32_t louvain_tile_load(const uint32_t *x, uint64_t count, uint32_t b, uint32_t v[4]) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t i = (uint64_t)b * kLouvainScanTile + threadIdx.x * 4u + k;
        v[k] = i < count ? x[i] : 0u;
        sum += v[k];
    }
    return sum;
}

__global__ __launch_bounds__(256) void louvain_scan_tile_kernel(const uint32_t *x, uint64_t count, uint32_t *tile) {
    __shared__ uint32_t s[256];
    uint32_t v[4], sum;
    louvain_block_scan(louvain_tile_load(x, count, blockIdx.x, v), s, &sum);
    if (threadIdx.x == 0) tile[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void louvain_scan_top_kernel(uint32_t *tile, uint32_t tiles, uint32_t *total) {
    __shared__ uint32_t s[256];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < tiles; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        uint32_t sum;
        const uint32_t before = louvain_block_scan(b < tiles ? tile[b] : 0u, s, &sum);
        if (b < tiles) tile[b] = carry + before;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void louvain_scan_apply_kernel(uint32_t *x, uint64_t count, const uint32_t *tile) {
    __shared__ uint32_t s[256];
    uint32_t v[4], sum;
    uint32_t at = tile[blockIdx.x] + louvain_block_scan(louvain_tile_load(x, count, blockIdx.x, v), s, &sum);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t i = (uint64_t)blockIdx.x * kLouvainScanTile + threadIdx.x * 4u + k;
        if (i < count) x[i] = at;
        at += v[k];
    }
}

// a node's renumbered community (into next), and per community: members, nonzeros of their rows, k and the members' loops
__global__ __launch_bounds__(256) void louvain_member_count_kernel(const LouvainArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const uint32_t C = a.newid[a.kept[i]];
    a.next[i] = C;
    atomicAdd(&a.ccount[C], 1u);
    atomicAdd(&a.orowbeg[C], a.rowend[i] - a.rowbeg[i]);
    atomicAdd(&a.ok[C], a.k[i]);
    if (a.loop[i]) atomicAdd(&a.oloop[C], a.loop[i]);
}

__global__ __launch_bounds__(256) void louvain_member_fill_kernel(const LouvainArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const uint32_t C = a.next[i];
    a.members[a.mstart[C] + atomicAdd(&a.size[C], 1u)] = (uint32_t)i;  // (size: the cursors, zeroed by the host)
}

__global__ __launch_bounds__(256) void louvain_relabel_kernel(const LouvainArgs a) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < a.n) a.vlabel[v] = a.next[a.vlabel[v]];
}

__global__ __launch_bounds__(256) void louvain_iota_kernel(uint32_t *x, uint32_t n) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) x[v] = (uint32_t)v;
}

// ---- the agreement of two labellings -----------------------------------------------------------------------------------------------
struct AgreeArgs {
    const uint32_t *a, *b;
    uint32_t *cells;                 // ka x kb cells, then ka row sums, then kb column sums
    unsigned long long *sums;        // [0] N, [1..3] sum of C(x, 2) over cells / rows / columns, [4..6] their nonzero counts
    double *pieces;                  // the piece sums of the three, one after the other; then flog(N)
    uint64_t cells_count;
    uint32_t n, ka, kb;
};

__global__ __launch_bounds__(256) void agree_count_kernel(const AgreeArgs g) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t x = v < g.n ? g.a[v] : F2V_LABEL_NONE, y = v < g.n ? g.b[v] : F2V_LABEL_NONE;
    const bool both = x != F2V_LABEL_NONE && y != F2V_LABEL_NONE;
    if (both) {
        atomicAdd(&g.cells[(uint64_t)x * g.kb + y], 1u);
        atomicAdd(&g.cells[g.cells_count + x], 1u);
        atomicAdd(&g.cells[g.cells_count + g.ka + y], 1u);
    }
    const unsigned long long mask = __ballot(both);  // N: one add per wavefront
    if (mask && (threadIdx.x & 63u) == 0) atomicAdd(g.sums + 0, (unsigned long long)__popcll(mask));
}

// which: 0 the cells, 1 the row sums, 2 the column sums.  One lane per piece of 1024 consecutive values, summed from +0 in order.
__global__ __launch_bounds__(256) void agree_piece_kernel(const AgreeArgs g, uint32_t which, uint64_t first, uint64_t count, uint64_t piece0) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x, pieces = (count + kAgreePiece - 1) / kAgreePiece;
    unsigned long long comb = 0, nonzero = 0;
    if (p < pieces) {
        const uint32_t *x = g.cells + first + p * kAgreePiece;
        const uint32_t m = (uint32_t)(count - p * kAgreePiece < kAgreePiece ? count - p * kAgreePiece : kAgreePiece);
        double s = 0.0;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t v = x[i];
            if (v == 0) continue;
            const double f = (double)v;
            s = s + f * exact_flog(f);
            comb += (unsigned long long)v * (v - 1u) / 2u;
            nonzero++;
        }
        g.pieces[piece0 + p] = s;
    }
    if (comb) atomicAdd(g.sums + 1 + which, comb);
    if (nonzero) atomicAdd(g.sums + 4 + which, nonzero);
}

__global__ void agree_log_kernel(const AgreeArgs g, uint64_t at) {
    const unsigned long long N = g.sums[0];
    g.pieces[at] = N ? exact_flog((double)N) : 0.0;
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_LOUVAIN_HIP_H_
