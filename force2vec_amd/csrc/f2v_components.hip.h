// f2v_components.hip.h -- connected components, spanning forests and induced subgraphs on gfx950 (definitions in include/f2v.h:
// components and spanning forests).
//
// Integers only, and every result is unique by its definition (a minimum label, the spanning forest of a strict total order), so it is
// the same bits under any schedule.  All kernels that walk nonzeros walk PIECES: a row of at most kCcPiece nonzeros is one wavefront's,
// a longer row is cut into pieces of kCcPiece nonzeros (a list the host builds once per handle from rowptr alone), each a wavefront's of
// its own, so a hub costs a round no more than its share of the nonzeros.  Two label arrays: L, the flattened labels a round reads and
// nothing writes while it is read, and P, the parents the round hooks and then flattens; a round ends with L = P.
//   cc_hook_kernel      a wavefront per piece: a nonzero whose ends carry different labels lowers P[the larger label] to the smaller
//                       one (32-bit atomicMin behind a plain read that spares most of them; an edge stored in one direction only
//                       hooks like any other: the rule is symmetric.  One atomic per piece for the nonzeros that aim at P[L[u]]
//                       measured the same and needed the symmetry check: not kept);
//   cc_jump_kernel      a thread per vertex: up to kCcJumps steps towards the root, then P[v] = where it got to; sets a word where a
//                       thread stopped short of a root (the host launches it again: one word read per launch);
//   cc_size_kernel / cc_stat_kernel   a thread per vertex: size[L[v]] += 1, one atomic per distinct label among a wavefront's non-roots
//                       (a lane per vertex adding to the one word of a giant component measured 7 ms more on RMAT-20); then sizes_out, the number of roots, of vertices alone and
//                       the largest size with the lowest label (one 64-bit atomicMax of size * 2^32 + ~label per wavefront);
//   cc_edges_kernel     a wavefront per piece: the distinct pairs -- a nonzero that differs from its predecessor, counted at its lower
//                       end, or at its upper end where the lower end's row does not hold it (binary search);
//   forest_key_kernel   Boruvka, step one: the best shifted key among a component's nonzeros whose other end lies in another component
//                       -- a maximum over the wavefront, then one 64-bit atomicMax per piece (the least forest takes the complement
//                       of key and pair, so one maximum serves both).  Where the CSR is not structurally symmetric every such nonzero
//                       also proposes itself to the OTHER end's component, whose rows may not hold it;
//   forest_pair_kernel  step two: among the nonzeros that match the component's key, the best packed pair a * 2^32 + b;
//   forest_hook_kernel  a thread per vertex: a root that found a pair hooks to the root at its other end and appends the pair to the
//                       forest; where two roots chose the same pair the lower one stays a root.  Everything else keeps its parent;
//   forest_mark_kernel  a wavefront per piece: flag[q] = the nonzero's pair is in the (sorted) forest, by binary search: set in both
//                       stored directions and on every duplicate;
//   sub_count_kernel / sub_fill_kernel   the induced subgraph: a wavefront per row counts, then writes its kept nonzeros under their
//                       new ids (ranks by ballot); the two 64-bit prefix sums between them are those of f2v_linkpairs.hip.h.
// Plain launches, no in-grid waits, no float atomics.
#ifndef F2V_COMPONENTS_HIP_H_
#define F2V_COMPONENTS_HIP_H_

#include "f2v.h"
#include "f2v_kernels.hip.h"
#include "f2v_linkpairs.hip.h"
#include "f2v_nearest.hip.h"

namespace f2v {
#ifdef F2V_TEST_HOOKS
inline namespace selftest {
#endif

constexpr uint32_t kCcPiece = 256;  // nonzeros of a row that one wavefront walks; a longer row is cut into pieces
constexpr uint32_t kCcJumps = 16;   // steps a thread of cc_jump_kernel takes towards its root
constexpr uint32_t kSubDropped = 0xFFFFFFFFu;  // new_id of a vertex that is not kept

struct CcItem {
    uint32_t u, lo, hi;  // nonzeros lo .. hi - 1 of row u
};

struct CcArgs {
    const uint32_t *rowptr, *colids;
    const CcItem *items;               // the pieces of the rows longer than kCcPiece
    uint32_t n, nitems;
    const uint32_t *L;                 // flattened labels: read only while a round's kernels run
    uint32_t *P;                       // parents: hooked, then flattened
    uint32_t *size, *sizes_out;
    unsigned long long *sums;          // [0] a round hooked / found a pair, [1] a jump stopped short, [2] distinct pairs, [3] roots,
                                       // [4] vertices alone, [5] size * 2^32 + ~label of the largest, [6] forest pairs so far
    // spanning forest
    unsigned long long *best1, *best2; // per root: the best shifted key, the best packed pair (0: none)
    unsigned long long *forest;        // the forest's packed pairs: appended by the hooks, sorted at the end
    uint8_t *flag;                     // per nonzero: its pair is in the forest
    uint64_t se;
    uint32_t shift, greatest, both;    // 64 - bits; both: the CSR is not symmetric, nonzeros propose to both ends
    uint64_t forest_count;
};

// f(u, row start, lo, hi) for every piece, a wavefront each (grid stride); 256 lanes a workgroup
template <class F>
__device__ __forceinline__ void cc_for_pieces(const CcArgs &a, F f) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t units = (uint64_t)a.n + a.nitems;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + wave; w < units; w += (uint64_t)gridDim.x * 4) {
        if (w < a.n) {
            const uint32_t u = (uint32_t)w, lo = a.rowptr[u], hi = a.rowptr[u + 1];
            if (hi - lo > kCcPiece) continue;  // its pieces follow
            f(u, lo, lo, hi);
        } else {
            const CcItem it = a.items[w - a.n];
            f(it.u, a.rowptr[it.u], it.lo, it.hi);
        }
    }
}

__device__ __forceinline__ unsigned long long cc_wave_max(unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long y = __shfl_xor(x, d);
        x = y > x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(256) void cc_iota_kernel(uint32_t *L, uint32_t *P, uint32_t n) {
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < n; v += (uint64_t)gridDim.x * 256u) L[v] = P[v] = (uint32_t)v;
}

__global__ __launch_bounds__(256) void cc_hook_kernel(const CcArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    bool any = false;
    cc_for_pieces(a, [&](uint32_t u, uint32_t, uint32_t lo, uint32_t hi) {
        const uint32_t lu = a.L[u];
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            if (lane >= hi - q0) continue;
            const uint32_t lv = a.L[a.colids[q0 + lane]];
            if (lv == lu) continue;
            const uint32_t up = lu > lv ? lu : lv, down = lu > lv ? lv : lu;
            if (a.P[up] > down) atomicMin(&a.P[up], down);  // (the read only spares atomics: P never rises)
            any = true;
        }
    });
    if (__ballot(any) && lane == 0) a.sums[0] = 1ull;
}

__global__ __launch_bounds__(256) void cc_jump_kernel(const CcArgs a) {
    bool shortfall = false;
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < a.n; v += (uint64_t)gridDim.x * 256u) {
        const uint32_t first = a.P[v];
        uint32_t p = first, g = a.P[p];
        for (uint32_t k = 0; k < kCcJumps && g != p; k++) {  // (another thread's store only ever names an ancestor)
            p = g;
            g = a.P[p];
        }
        if (p != first) a.P[v] = p;
        shortfall = shortfall || g != p;
    }
    if (__ballot(shortfall) && (threadIdx.x & 63u) == 0) a.sums[1] = 1ull;
}

// size[L[v]] += 1 for every v.  A root adds for itself (no two roots share a word); the other lanes of a wavefront mostly name one
// root -- the ids of a large component come in runs -- so they add once per distinct label among them, not once per lane
__global__ __launch_bounds__(256) void cc_size_kernel(const CcArgs a) {
    const uint64_t rounds = ((uint64_t)a.n + 255u) / 256u;
    for (uint64_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const uint64_t v = r * 256u + threadIdx.x;
        const bool in = v < a.n;
        const uint32_t l = in ? a.L[v] : 0u;
        if (in && l == (uint32_t)v) atomicAdd(&a.size[l], 1u);
        bool todo = in && l != (uint32_t)v;
        for (unsigned long long left = __ballot(todo); left; left = __ballot(todo)) {
            const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)l, __builtin_ctzll(left));
            const unsigned long long same = __ballot(todo && l == first);
            if (todo && l == first) {
                todo = false;
                if (link_lanes_below(same) == 0) atomicAdd(&a.size[first], (uint32_t)__popcll(same));
            }
        }
    }
}

__global__ __launch_bounds__(256) void cc_stat_kernel(const CcArgs a) {
    unsigned long long roots = 0, alone = 0, top = 0;
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < a.n; v += (uint64_t)gridDim.x * 256u) {
        const uint32_t l = a.L[v], s = a.size[l];
        if (a.sizes_out) a.sizes_out[v] = s;
        alone += s == 1u;
        if (l == (uint32_t)v) {
            roots++;
            const unsigned long long mine = ((unsigned long long)s << 32) | (0xFFFFFFFFu - l);  // ties to the lowest label
            top = mine > top ? mine : top;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        roots += __shfl_xor(roots, d);
        alone += __shfl_xor(alone, d);
    }
    top = cc_wave_max(top);
    if ((threadIdx.x & 63u) == 0) {
        if (roots) atomicAdd(a.sums + 3, roots);
        if (alone) atomicAdd(a.sums + 4, alone);
        if (top) atomicMax(a.sums + 5, top);
    }
}

__global__ __launch_bounds__(256) void cc_edges_kernel(const CcArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long pairs = 0;
    cc_for_pieces(a, [&](uint32_t u, uint32_t start, uint32_t lo, uint32_t hi) {
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            const bool in = lane < hi - q0;
            const uint32_t q = q0 + lane, v = in ? a.colids[q] : 0u;
            const bool nb = in && v != u && (q == start || a.colids[q - 1] != v);
            const bool mine = nb && (v > u || !nn_is_neighbour(a.rowptr, a.colids, v, u));
            pairs += (uint32_t)__popcll(__ballot(mine));
        }
    });
    if (lane == 0 && pairs) atomicAdd(a.sums + 2, pairs);
}

// ---- spanning forest --------------------------------------------------------------------------------------------------------------
// the order's two words for the nonzero (u, v), u != v: larger is better for either forest
__device__ __forceinline__ unsigned long long forest_pair(const CcArgs &a, uint32_t u, uint32_t v) {
    const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
    const unsigned long long p = ((unsigned long long)lo << 32) | hi;
    return a.greatest ? p : ~p;  // never 0: lo < hi <= 2^32 - 1
}

__device__ __forceinline__ unsigned long long forest_key(const CcArgs &a, uint32_t u, uint32_t v) {
    const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
    const unsigned long long k = mix64(a.se ^ (((uint64_t)lo << 32) | hi)) >> a.shift;
    return a.greatest ? k : ~k;
}

__global__ __launch_bounds__(256) void forest_key_kernel(const CcArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    cc_for_pieces(a, [&](uint32_t u, uint32_t, uint32_t lo, uint32_t hi) {
        const uint32_t lu = a.L[u];
        unsigned long long best = 0;  // (a piece without an outgoing nonzero, or whose best is 0, has nothing to add to a word that starts at 0)
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            if (lane >= hi - q0) continue;
            const uint32_t v = a.colids[q0 + lane], lv = a.L[v];
            if (lv == lu) continue;
            const unsigned long long k = forest_key(a, u, v);
            best = k > best ? k : best;
            if (a.both && a.best1[lv] < k) atomicMax(&a.best1[lv], k);
        }
        best = cc_wave_max(best);
        if (lane == 0 && a.best1[lu] < best) atomicMax(&a.best1[lu], best);
    });
}

__global__ __launch_bounds__(256) void forest_pair_kernel(const CcArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    cc_for_pieces(a, [&](uint32_t u, uint32_t, uint32_t lo, uint32_t hi) {
        const uint32_t lu = a.L[u];
        const unsigned long long want = a.best1[lu];
        unsigned long long best = 0;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            if (lane >= hi - q0) continue;
            const uint32_t v = a.colids[q0 + lane], lv = a.L[v];
            if (lv == lu) continue;
            const unsigned long long k = forest_key(a, u, v), p = forest_pair(a, u, v);
            if (k == want) best = p > best ? p : best;
            if (a.both && k == a.best1[lv] && a.best2[lv] < p) atomicMax(&a.best2[lv], p);
        }
        best = cc_wave_max(best);
        if (lane == 0 && a.best2[lu] < best) atomicMax(&a.best2[lu], best);
    });
}

__global__ __launch_bounds__(256) void forest_hook_kernel(const CcArgs a) {
    bool found = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t r = (uint32_t)i, l = a.L[r];
        uint32_t parent = l;
        const unsigned long long mine = l == r ? a.best2[r] : 0ull;
        if (mine) {
            found = true;
            const unsigned long long pair = a.greatest ? mine : ~mine;
            const uint32_t la = a.L[(uint32_t)(pair >> 32)], lb = a.L[(uint32_t)pair], other = la == r ? lb : la;
            if (!(a.best2[other] == mine && r < other)) {  // two roots with one pair: the lower one stays a root
                parent = other;
                a.forest[atomicAdd(a.sums + 6, 1ull)] = pair;  // (at most n - 1 hooks in all: every hook removes a root)
            }
        }
        a.P[r] = parent;
    }
    if (__ballot(found) && (threadIdx.x & 63u) == 0) a.sums[0] = 1ull;
}

__device__ __forceinline__ bool forest_holds(const unsigned long long *forest, uint64_t count, unsigned long long pair) {
    uint64_t lo = 0, hi = count;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (forest[mid] < pair) lo = mid + 1;
        else hi = mid;
    }
    return lo < count && forest[lo] == pair;
}

__global__ __launch_bounds__(256) void forest_mark_kernel(const CcArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    cc_for_pieces(a, [&](uint32_t u, uint32_t, uint32_t lo, uint32_t hi) {
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            if (lane >= hi - q0) continue;
            const uint32_t q = q0 + lane, v = a.colids[q], x = u < v ? u : v, y = u < v ? v : u;
            a.flag[q] = v != u && forest_holds(a.forest, a.forest_count, ((unsigned long long)x << 32) | y) ? 1 : 0;
        }
    });
}

// ---- induced subgraph -------------------------------------------------------------------------------------------------------------
struct SubArgs {
    const uint32_t *rowptr, *colids;
    const uint8_t *keep;
    uint32_t *kept, *cnt;                       // per vertex: 1 if kept, its kept nonzeros
    const unsigned long long *id_at, *row_at;   // per vertex: its rank among the kept, the index of its first kept nonzero
    unsigned long long *sums;                   // [0] rows, [1] nonzeros
    uint32_t *rowptr_out, *colids_out, *new_id;
    uint32_t n;
};

__global__ __launch_bounds__(256) void sub_count_kernel(const SubArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long rows = 0, nnz = 0;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const bool mine = a.keep[u] != 0;
        uint32_t c = 0;
        if (mine) {
            const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
            for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
                const bool in = lane < hi - q0;
                c += (uint32_t)__popcll(__ballot(in && a.keep[a.colids[q0 + lane]] != 0));
            }
        }
        if (lane == 0) {
            a.kept[u] = mine ? 1u : 0u;
            a.cnt[u] = c;
        }
        rows += mine ? 1u : 0u;
        nnz += c;
    }
    if (lane == 0) {
        if (rows) atomicAdd(a.sums + 0, rows);
        if (nnz) atomicAdd(a.sums + 1, nnz);
    }
}

__global__ __launch_bounds__(256) void sub_fill_kernel(const SubArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t u = blockIdx.x * 4 + wave; u < a.n; u += gridDim.x * 4) {
        const bool mine = a.keep[u] != 0;
        if (lane == 0) a.new_id[u] = mine ? (uint32_t)a.id_at[u] : kSubDropped;
        if (!mine) continue;
        const uint32_t lo = a.rowptr[u], hi = a.rowptr[u + 1];
        uint64_t at = a.row_at[u];
        if (lane == 0) a.rowptr_out[a.id_at[u]] = (uint32_t)at;
        for (uint32_t q0 = lo; q0 < hi; q0 += 64) {
            const bool in = lane < hi - q0;
            const uint32_t v = in ? a.colids[q0 + lane] : 0u;
            const bool take = in && a.keep[v] != 0;
            const unsigned long long mask = __ballot(take);
            if (take) a.colids_out[at + link_lanes_below(mask)] = (uint32_t)a.id_at[v];
            at += (uint32_t)__popcll(mask);
        }
    }
}

#ifdef F2V_TEST_HOOKS
}  // inline namespace selftest
#endif
}  // namespace f2v
#endif  // F2V_COMPONENTS_HIP_H_
