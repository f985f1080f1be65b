// f2v_linkpairs.hip.h -- the link-prediction pair set on gfx950 (definition in include/f2v.h: link prediction pairs).
//
// Integers only: the result is a function of (CSR, ratio, seed), whatever the launch shapes.
//   link_count_kernel     one wavefront per vertex (grid stride), lanes over the row: |N(u)| and p(u) by "differs from its predecessor"
//                         ballots, total(u) by the rule; the call's sums go to four 64-bit words, one integer atomic per wavefront;
//   link_scan_*_kernel    exclusive prefix sums of p + total in 64 bits: tile sums (1024 vertices a workgroup), one workgroup over the
//                         tile sums, then the tiles again with their base;
//   link_positive_kernel  one wavefront per vertex: positive k of u goes to place perm(offset(u) + k);
//   link_short_kernel     total(u) <= "link_short_max": one wavefront per vertex (grid stride over the placement order), 64 candidates
//                         t a round, one a lane.  A lane's candidate is tested against u, against the row (binary search), against
//                         the accepted set -- a list in LDS, read by all lanes at once -- and against the lower lanes' candidates
//                         (a lower lane's candidate that was itself refused is refused for a reason this one shares, so all lower
//                         lanes are compared).  Survivors are ranked by ballot and mbcnt; the round is cut at total(u);
//   link_long_kernel      longer lists: one workgroup per vertex, a candidate a lane and round.  The accepted set is an open-addressing
//                         table of (key, the t that brought it) -- in LDS up to kLinkLdsSlots slots (256 lanes), else in the workspace
//                         (1024 lanes: a round is one chain of dependent loads and atomics however wide it is, and the vertex with
//                         the most negatives decides how long the call lasts).  Every candidate that is neither u nor a neighbour claims its key's slot (integer
//                         compare-and-swap) and lowers the slot's t to its own (integer minimum): a slot whose t lies before the round
//                         holds an earlier round's negative; after the barrier the lane whose t the slot holds is the one that wins.
//                         Ranks in t order from ballots and the wavefronts' counts.
// Both forms write negative k of u straight to place perm(offset(u) + p(u) + k) of the three result arrays; a vertex's index of its
// last accepted candidate + 1 is added to the call's `candidates`.  Plain launches, no in-grid waits, no float atomics.
#ifndef F2V_LINKPAIRS_HIP_H_
#define F2V_LINKPAIRS_HIP_H_

#include "f2v.h"
#include "f2v_kernels.hip.h"
#include "f2v_nearest.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kLinkShortLimit = 1024;  // the largest "link_short_max": 4 KiB of LDS per wavefront
constexpr uint32_t kLinkLongThreads = 256;  // candidates per round of the long form with its table in LDS
constexpr uint32_t kLinkWideThreads = 1024; // ... and with its table in the workspace
constexpr uint32_t kLinkLdsSlots = 8192;    // the largest table kept in LDS: 64 KiB of keys and t's
constexpr uint32_t kLinkScanTile = 1024;    // vertices per workgroup of the scan
constexpr uint32_t kLinkEmpty = 0xFFFFFFFFu;  // no key (ids are below n <= 2^32 - 1), and the t of a slot nobody has claimed

// slots of a vertex's table: a power of two, at most half full after a last round that claims up to 1024 keys past total(u)
__host__ __device__ inline uint64_t link_slots(uint32_t total) {
    uint64_t s = 2 * kLinkWideThreads;
    while (s < 2 * (uint64_t)total + 2 * kLinkWideThreads) s <<= 1;
    return s;
}

struct LinkArgs {
    const uint32_t *rowptr, *colids;
    uint32_t *p, *total;             // per vertex: p(u), total(u)
    unsigned long long *offset;      // per vertex: the index of its first item
    unsigned long long *tile;        // the scan's tile sums
    unsigned long long *sums;        // [0] positives, [1] negatives, [2] capped, [3] candidates
    const uint32_t *order;           // this launch's vertices, longest list first
    const unsigned long long *table_at;  // long form in the workspace: per vertex of this launch the first slot of its table
    uint32_t *keys;                  // ... and the tables: the keys of all of them, then -- table_words further -- the t's
    uint64_t table_words;
    uint32_t *u_out, *v_out;
    uint8_t *y_out;
    uint64_t s1, s2;                 // mix64(seed), mix64(mix64(seed))
    uint64_t M, mask;                // the shuffle: items, 2^half - 1
    uint32_t half;
    uint32_t n, ratio, count;        // count: vertices of this launch
    uint32_t short_max;              // LDS words per wavefront of link_short_kernel
    uint32_t slots;                  // long form in LDS: slots of this launch's tables
};

// place of item i: four Feistel rounds on 2 x half bits, walked until the value is an item index
__device__ __forceinline__ uint64_t link_perm(const LinkArgs &a, uint64_t i) {
    uint64_t x = i;
    do {
        uint64_t L = x >> a.half, R = x & a.mask;
#pragma unroll
        for (uint64_t r = 0; r < 4; r++) {
            const uint64_t f = mix64(a.s2 ^ ((r << 32) + R)) & a.mask;
            const uint64_t nr = L ^ f;
            L = R;
            R = nr;
        }
        x = (L << a.half) | R;
    } while (x >= a.M);
    return x;
}

__device__ __forceinline__ void link_store(const LinkArgs &a, uint64_t item, uint32_t u, uint32_t v, uint8_t y) {
    const uint64_t at = link_perm(a, item);
    a.u_out[at] = u;
    a.v_out[at] = v;
    a.y_out[at] = y;
}

__device__ __forceinline__ uint32_t link_candidate(const LinkArgs &a, uint64_t hu, uint32_t t) { return (uint32_t)(mix64(hu + t) % (uint64_t)a.n); }

__device__ __forceinline__ uint32_t link_lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(256) void link_count_kernel(const LinkArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long pos = 0, neg = 0, capped = 0;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        uint32_t nu = 0, p = 0;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {  // (hi - q0 keeps the bound where q0 + lane would wrap)
            const bool in = lane < hi - q0;
            const uint32_t q = q0 + lane, v = in ? a.colids[q] : 0u;
            const bool nb = in && v != u && (q == lo || a.colids[q - 1] != v);
            nu += (uint32_t)__popcll(__ballot(nb));
            p += (uint32_t)__popcll(__ballot(nb && v > u));
        }
        const unsigned long long want = (unsigned long long)a.ratio * p, room = (a.n - 1u - nu) / 2u;
        const uint32_t total = (uint32_t)(want < room ? want : room);
        if (lane == 0) {
            a.p[u] = p;
            a.total[u] = total;
        }
        pos += p;
        neg += total;
        capped += room < want ? 1u : 0u;
    }
    if (lane == 0) {
        if (pos) atomicAdd(a.sums + 0, pos);
        if (neg) atomicAdd(a.sums + 1, neg);
        if (capped) atomicAdd(a.sums + 2, capped);
    }
}

// the exclusive prefix sums of a workgroup's 256 values, and their sum
__device__ __forceinline__ unsigned long long link_block_scan(unsigned long long x, unsigned long long *s, unsigned long long *sum) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    s[t] = x;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const unsigned long long y = t >= d ? s[t - d] : 0ull;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    *sum = s[255];
    return s[t] - x;
}

// the four items of thread t in tile b, summed
__device__ __forceinline__ unsigned long long link_tile_load(const LinkArgs &a, uint32_t b, unsigned long long x[4]) {
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t v = (uint64_t)b * kLinkScanTile + threadIdx.x * 4u + k;
        x[k] = v < a.n ? (unsigned long long)a.p[v] + a.total[v] : 0ull;
        sum += x[k];
    }
    return sum;
}

__global__ __launch_bounds__(256) void link_scan_tile_kernel(const LinkArgs a) {
    __shared__ unsigned long long s[256];
    unsigned long long x[4], sum;
    link_block_scan(link_tile_load(a, blockIdx.x, x), s, &sum);
    if (threadIdx.x == 0) a.tile[blockIdx.x] = sum;
}

// tile[b] = the sum of the tiles before b; one workgroup, 256 tiles at a time
__global__ __launch_bounds__(256) void link_scan_top_kernel(const LinkArgs a, uint32_t tiles) {
    __shared__ unsigned long long s[256];
    unsigned long long carry = 0;
    for (uint32_t b0 = 0; b0 < tiles; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        unsigned long long sum;
        const unsigned long long before = link_block_scan(b < tiles ? a.tile[b] : 0ull, s, &sum);
        if (b < tiles) a.tile[b] = carry + before;
        carry += sum;
    }
}

__global__ __launch_bounds__(256) void link_scan_apply_kernel(const LinkArgs a) {
    __shared__ unsigned long long s[256];
    unsigned long long x[4], sum;
    unsigned long long at = a.tile[blockIdx.x] + link_block_scan(link_tile_load(a, blockIdx.x, x), s, &sum);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t v = (uint64_t)blockIdx.x * kLinkScanTile + threadIdx.x * 4u + k;
        if (v < a.n) a.offset[v] = at;
        at += x[k];
    }
}

__global__ __launch_bounds__(256) void link_positive_kernel(const LinkArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        if (a.p[u] == 0) continue;
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        uint64_t at = a.offset[u];
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            const bool in = lane < hi - q0;
            const uint32_t q = q0 + lane, v = in ? a.colids[q] : 0u;
            const bool is = in && v > u && (q == lo || a.colids[q - 1] != v);
            const unsigned long long mask = __ballot(is);
            if (is) link_store(a, at + link_lanes_below(mask), u, v, 1);
            at += (uint32_t)__popcll(mask);
        }
    }
}

__global__ __launch_bounds__(256) void link_short_kernel(const LinkArgs a) {
    extern __shared__ uint32_t link_smem[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *set = link_smem + (size_t)wave * a.short_max;  // the vertex's negatives so far
    unsigned long long drawn = 0;
    for (uint32_t w = blockIdx.x * 4 + wave; w < a.count; w += gridDim.x * 4) {
        const uint32_t u = a.order[w], total = a.total[u];
        const uint64_t hu = mix64(a.s1 ^ (uint64_t)u), at = a.offset[u] + a.p[u];
        uint32_t acc = 0;
        for (uint32_t base = 0; acc < total; base += 64) {
            const uint32_t t = base + lane, cand = link_candidate(a, hu, t);
            bool ok = cand != u && !nn_is_neighbour(a.rowptr, a.colids, u, cand);
            for (uint32_t j = 0; j < acc; j++) ok = ok && set[j] != cand;
#pragma unroll 1
            for (uint32_t j0 = 0; j0 < 64; j0 += 8) {  // (eight lanes a step: all 63 at once would not fit the scalar registers)
#pragma unroll
                for (uint32_t j = j0; j < j0 + 8; j++) {
                    const uint32_t other = __builtin_amdgcn_readlane(cand, j);
                    ok = ok && !(j < lane && other == cand);
                }
            }
            const unsigned long long mask = __ballot(ok);
            const uint32_t rank = acc + link_lanes_below(mask);
            if (ok && rank < total) {
                set[rank] = cand;
                link_store(a, at + rank, u, cand, 0);
            }
            const unsigned long long last = __ballot(ok && rank + 1 == total);
            if (last) drawn += base + (uint32_t)__builtin_ctzll(last) + 1u;
            acc += (uint32_t)__popcll(mask);
            nn_wave_sync();  // (the set is read by every lane in the next round)
        }
        nn_wave_sync();  // (... and reused by the next vertex)
    }
    if (lane == 0 && drawn) atomicAdd(a.sums + 3, drawn);
}

template <bool WORKSPACE>
__device__ __forceinline__ auto link_table(const LinkArgs &a, uint32_t *lds) {
    if constexpr (WORKSPACE) return a.keys + a.table_at[blockIdx.x];
    else return lds;
}

template <bool WORKSPACE>
__global__ __launch_bounds__(WORKSPACE ? kLinkWideThreads : kLinkLongThreads) void link_long_kernel(const LinkArgs a) {
    constexpr uint32_t kThreads = WORKSPACE ? kLinkWideThreads : kLinkLongThreads, kWaves = kThreads / 64;
    extern __shared__ uint32_t link_smem[];  // the wavefronts' counts of two rounds; LDS form: the keys and the t's behind them
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t u = a.order[blockIdx.x], total = a.total[u];
    uint32_t(*wave_count)[kWaves] = reinterpret_cast<uint32_t(*)[kWaves]>(link_smem);
    const uint32_t slots = WORKSPACE ? (uint32_t)link_slots(total) : a.slots;  // (a table has at most 2^32 / 2 slots: total < n / 2)
    const uint32_t slot_mask = slots - 1u, shift = 32u - (uint32_t)__builtin_ctz(slots);
    auto *keys = link_table<WORKSPACE>(a, link_smem + 2 * kWaves), *tmin = keys + (WORKSPACE ? a.table_words : slots);
    if (!WORKSPACE) {  // (the workspace's tables are filled with kLinkEmpty by the host)
        for (uint32_t i = tid; i < 2 * slots; i += kThreads) keys[i] = kLinkEmpty;
        __syncthreads();
    }
    const uint64_t hu = mix64(a.s1 ^ (uint64_t)u), at = a.offset[u] + a.p[u];
    uint32_t acc = 0, round = 0;
    for (uint32_t base = 0; acc < total; base += kThreads, round ^= 1u) {
        const uint32_t t = base + tid, cand = link_candidate(a, hu, t);
        bool ok = cand != u && !nn_is_neighbour(a.rowptr, a.colids, u, cand);
        uint32_t s = 0;
        if (ok) {
            s = (cand * 0x9E3779B1u) >> shift;
            for (;;) {
                const uint32_t old = atomicCAS(&keys[s], kLinkEmpty, cand);
                if (old == kLinkEmpty || old == cand) break;
                s = (s + 1u) & slot_mask;
            }
            ok = atomicMin(&tmin[s], t) >= base;  // below base: the key is an earlier round's negative
        }
        __syncthreads();
        if (ok) ok = (WORKSPACE ? __hip_atomic_load(&tmin[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tmin[s]) == t;
        const unsigned long long mask = __ballot(ok);
        if (lane == 0) wave_count[round][wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t rank = acc + link_lanes_below(mask), all = 0;
#pragma unroll
        for (uint32_t k = 0; k < kWaves; k++) {
            const uint32_t cnt = wave_count[round][k];
            rank += k < wave ? cnt : 0u;
            all += cnt;
        }
        if (ok && rank < total) link_store(a, at + rank, u, cand, 0);
        if (ok && rank + 1 == total) atomicAdd(a.sums + 3, (unsigned long long)t + 1ull);
        acc += all;
    }
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_LINKPAIRS_HIP_H_
